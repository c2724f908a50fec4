"""AsyncAmdLM's auto_kv_span on the CPU: the constructor's checks, and that the default changes nothing."""
import pytest

from tests.test_kv_chunk_cpu import _gpt2, gold  # noqa: F401  (the golden GPT-2 on the CPU restatement engine)


def test_constructor_takes_and_validates_auto_kv_span(gold):  # noqa: F811
    akv = _gpt2(gold, auto_kv_rows=10, auto_kv_cap=64, auto_kv_chunk=4, auto_kv_span=48)[0]._auto_kv
    assert (akv.chunk, akv.span) == (4, 48)
    for kw in (dict(auto_kv_rows=4), dict(auto_kv_rows=4, auto_kv_chunk=8)):
        akv = _gpt2(gold, **kw)[0]._auto_kv
        assert akv.span is None and akv.chunk == kw.get("auto_kv_chunk", 1)  # None: the limit stays auto_kv_chunk's
    for bad in (16, 129, 0, -1, 32.0, True, "32"):
        with pytest.raises(ValueError):
            _gpt2(gold, auto_kv_rows=10, auto_kv_span=bad)
    with pytest.raises(ValueError):
        _gpt2(gold, auto_kv_span=32)  # no rows to share prefixes in
    with pytest.raises(ValueError):
        _gpt2(gold, auto_kv_rows=10, auto_kv_chunk=17, auto_kv_span=32)  # auto_kv_chunk keeps its own range
