"""`ByteDFA.from_regex` without a GPU: every supported construct against Python's `re` on the bytes pattern - `fullmatch` on
every string up to length 5 over the pattern's own bytes plus \\n and 0xff, and on 500 seeded random byte strings - and
every refused construct named in its ValueError."""
import itertools
import re

import numpy as np
import pytest

from genlm_backend_amd.constraints import ByteDFA

PATTERNS = [
    rb"",
    rb"abc",
    rb"a|b|cd",
    rb"(a|ab)(c|bcd)",
    rb"-?(0|[1-9][0-9]*)(\.[0-9]+)?",
    rb"a*b+c?",
    rb"(ab)*(?:cd)+e?",
    rb"((a|b)*c)+|()",
    rb"(a(b(c|d)*)?)+",
    rb"a{3}",
    rb"a{2,}b",
    rb"a{2,4}",
    rb"a{,2}b",
    rb"a{0}b{0,1}c{1,1}",
    rb"(ab|c){1,3}d",
    rb"a{}b{x{1,",
    rb".",
    rb".*a.{2}",
    rb"[abc]+",
    rb"[a-cx-z]*",
    rb"[^a-c]",
    rb"[^\n]b|[^ab\xff]",
    rb"[]a]+[^]b]",
    rb"[a\-c]+[-a][a-]",
    rb"\d+\D",
    rb"\w+\W\s\S",
    rb"[\d\s]+[^\w]",
    rb"[\Wa]b",
    rb"\x41\x0a\xff",
    rb"[\x00-\x1f\xfe-\xff]a",
    rb"\\\.\*\+\?\(\)\[\]\{\}\|\^\$\-\/",
    rb"\n\t\r",
    rb"a|",
    rb"(|a)b",
    rb"( yes| no| maybe)",
    "é+ü?",
    "[a-c]ß|日",
]
REFUSED = [
    (rb"^a", "anchor"), (rb"a$", "anchor"), (rb"\Aa", "anchor"), (rb"a\Z", "anchor"), (rb"\bfoo", "boundary"), (rb"a\B", "boundary"),
    (rb"(a)\1", "backreference"), (rb"(?P<n>a)(?P=n)", "named group"), (rb"(?P=n)", "backreference"), (rb"(?=a)a", "lookaround"),
    (rb"(?!a)b", "lookaround"), (rb"(?<=a)b", "lookaround"), (rb"(?<!a)b", "lookaround"), (rb"a*?", "lazy"), (rb"a+?", "lazy"),
    (rb"a??", "lazy"), (rb"a{2,3}?", "lazy"), (rb"a*+", "possessive"), (rb"a++", "possessive"), (rb"a{2}+", "possessive"),
    (rb"(?i)a", "inline flag"), (rb"(?s:a)", "inline flag"), (rb"(?#note)a", "comment"), (rb"(?>a)", "atomic"),
    (rb"(?(1)a|b)", "conditional"), (rb"a{1001}", "bound above 1000"), (rb"a{2,1001}", "bound above 1000"), (rb"a{3,2}", "maximum"),
    (rb"*a", "nothing to repeat"), (rb"(|*)", "nothing to repeat"), (rb"a**", "repeated quantifier"), (rb"a{2}{3}", "repeated quantifier"),
    (rb"(a", "unbalanced"), (rb"a)", "unbalanced"), (rb"[a", "unterminated"), (rb"[z-a]", "range"), (rb"[a-\d]", "range"),
    (rb"\q", r"\\q"), (rb"\0", "octal"), (rb"[\b]", "boundary"), (rb"\x4", r"\\x"), ("a\\", "backslash"),
]


def _bytes(pattern):
    return pattern.encode("utf-8") if isinstance(pattern, str) else pattern


@pytest.mark.parametrize("pattern", PATTERNS, ids=[repr(p) for p in PATTERNS])
def test_accepts_what_fullmatch_matches(pattern):
    dfa = ByteDFA.from_regex(pattern)
    rx = re.compile(_bytes(pattern))
    assert dfa.start == 0 and dfa.delta.dtype == np.int32 and dfa.reachable.all()
    ByteDFA(dfa.delta, dfa.accepting, dfa.start)  # the tables pass the class's own validation again
    # the pattern's own bytes - letters, digits and non-ASCII bytes first, at most six of them - plus \n, 0xff and a digit:
    # 9^5 strings at the most
    rank = lambda b: (0 if bytes([b]).isalnum() or b >= 128 else 1 if b in b"-. " else 2, b)
    alphabet = sorted(set(sorted(set(_bytes(pattern)), key=rank)[:6]) | {10, 255, 48})
    for n in range(6):
        for t in itertools.product(alphabet, repeat=n):
            s = bytes(t)
            want = rx.fullmatch(s) is not None
            assert dfa.accepts(s) == want, (pattern, s)
    rng = np.random.default_rng(len(_bytes(pattern)))
    pool = np.array(sorted(set(_bytes(pattern)) | {10, 255, 0, 65}), np.uint8)
    for k in range(500):
        src = pool if k % 2 else np.arange(256, dtype=np.uint8)
        s = bytes(rng.choice(src, int(rng.integers(0, 12))))
        assert dfa.accepts(s) == (rx.fullmatch(s) is not None), (pattern, s)


def test_a_str_pattern_is_its_utf8_bytes():
    assert ByteDFA.from_regex("日本").accepts("日本".encode()) and not ByteDFA.from_regex("日本").accepts("日".encode())
    d = ByteDFA.from_regex("é+")  # the quantifier repeats the last byte, as `re` reads the bytes pattern
    assert d.accepts(b"\xc3\xa9\xa9") and not d.accepts(b"\xc3\xa9\xc3\xa9")
    assert ByteDFA.from_regex(rb"( yes| no| maybe)").accepts(b" maybe")
    assert ByteDFA.from_regex(rb"\\\.\*\+\?\(\)\[\]\{\}\|\^\$\-\/").accepts(rb"\.*+?()[]{}|^$-/")
    for pattern, member in ((rb"\d+\D", b"12x"), (rb"\n\t\r", b"\n\t\r"), (rb"\x41\x0a\xff", b"A\n\xff"), (rb"a{}b{x{1,", b"a{}b{x{1,"),
                            (rb"\w+\W\s\S", b"a_9- x"), (rb"[\x00-\x1f\xfe-\xff]a", b"\xfea"), (rb"-?(0|[1-9][0-9]*)(\.[0-9]+)?", b"-10.25")):
        assert ByteDFA.from_regex(pattern).accepts(member), pattern
    assert ByteDFA.from_regex(b"").accepts(b"") and not ByteDFA.from_regex(b"").accepts(b"a")


@pytest.mark.parametrize("pattern,named", REFUSED, ids=[repr(p) for p, _ in REFUSED])
def test_refused_constructs_are_named(pattern, named):
    with pytest.raises(ValueError, match=named) as e:
        ByteDFA.from_regex(pattern)
    assert "position" in str(e.value)


def test_max_states():
    with pytest.raises(ValueError, match="max_states=1000"):
        ByteDFA.from_regex(rb"(a|b)*a(a|b){14}", max_states=1000)
    assert ByteDFA.from_regex(rb"(a|b)*a(a|b){3}", max_states=16).n_states == 16
    with pytest.raises(ValueError, match="max_states=15"):
        ByteDFA.from_regex(rb"(a|b)*a(a|b){3}", max_states=15)
    for bad in (0, -1, True, 2.5):
        with pytest.raises(ValueError, match="max_states"):
            ByteDFA.from_regex(rb"a", max_states=bad)
