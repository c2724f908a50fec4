"""Weight pushing (include/glb.h glb_dfa_backward / glb_dfa_push_weights), restated in NumPy: the same Jacobi sweeps and stop
rule in float32 and in float64, the push formulas in float32, and the automata and weights the tests push.  Test
infrastructure: the product never imports it."""
import numpy as np

NINF = np.float32(-np.inf)
LOG, MAX = "log", "max"
TOL = 2.0 ** -20


def sweep(delta, arc, fin, beta, semiring):
    """beta_{k+1} from beta_k, in beta's dtype: final[s] (+) (+)_b (arc[s, b] + beta_k[delta[s, b]])."""
    dt = beta.dtype
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = (arc.astype(dt) + beta[np.maximum(delta, 0)]).astype(dt)
        t[(delta < 0) | (delta >= len(beta))] = -np.inf
        m = np.maximum(t.max(axis=1), fin.astype(dt))
        if semiring == MAX:
            return m
        ms = np.where(np.isneginf(m), dt.type(0), m)  # (a state without a finite term: nothing is subtracted from -inf)
        tot = np.exp(t - ms[:, None]).astype(dt).sum(axis=1, dtype=dt) + np.exp(fin.astype(dt) - ms).astype(dt)
        return np.where(np.isneginf(m), dt.type(-np.inf), (ms + np.log(tot)).astype(dt)).astype(dt)


def changed(new, old, semiring, tol):
    """The stop rule: did some state move?  MAX: by anything; LOG: by more than tol * max(1, |new|); -inf to -inf: no."""
    if semiring == MAX:
        return bool((new != old).any())
    dt = new.dtype
    with np.errstate(invalid="ignore"):
        return bool((~(new == old) & (np.abs(new - old) > dt.type(tol) * np.maximum(dt.type(1), np.abs(new)))).any())


def backward(delta, arc, fin, semiring, tol=TOL, max_sweeps=4096, dtype=np.float32):
    """(beta, sweeps performed, converged): from beta_0 = final, sweeps until one leaves every state where it was - that
    sweep is counted and its result returned - or `max_sweeps` are done."""
    delta = np.asarray(delta, np.int64)
    beta = np.asarray(fin).astype(dtype)
    for k in range(1, max_sweeps + 1):
        new = sweep(delta, arc, fin, beta, semiring)
        moved = changed(new, beta, semiring, tol)
        beta = new
        if not moved:
            return beta, k, True
    return beta, max_sweeps, False


def fixed_point64(delta, arc, fin, semiring):
    """float64 beta at its fixed point (stop rule at tol = 1e-15)."""
    beta, _, ok = backward(delta, arc, fin, semiring, tol=1e-15, max_sweeps=4096, dtype=np.float64)
    assert ok
    return beta


def push(delta, arc, fin, beta):
    """(arc_out, final_out) float32: (arc + beta[next]) - beta[s] and final - beta[s]; all of a state with beta = -inf, and
    an arc delta does not have, are -inf."""
    delta = np.asarray(delta, np.int64)
    arc, fin, beta = np.asarray(arc, np.float32), np.asarray(fin, np.float32), np.asarray(beta, np.float32)
    dead = np.isneginf(beta)
    bs = np.where(dead, np.float32(0), beta)
    with np.errstate(invalid="ignore"):
        a = ((arc + beta[np.maximum(delta, 0)]).astype(np.float32) - bs[:, None]).astype(np.float32)
        f = (fin - bs).astype(np.float32)
    a[(delta < 0) | (delta >= len(beta)) | dead[:, None]] = NINF
    f[dead] = NINF
    return a, f


def substochastic_weights(delta, accepting, seed, mass=0.5):
    """(arc_logw, final_logw) float32: every state's arc probabilities sum to `mass`, an accepting state's final probability
    lies in [0.1, 0.5] - the iteration for the backward weights contracts with ratio <= mass."""
    rng = np.random.default_rng(seed)
    delta, accepting = np.asarray(delta), np.asarray(accepting, np.bool_)
    p = np.where(delta >= 0, 0.05 + rng.random(delta.shape), 0.0)
    tot = p.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        arc = np.where(delta >= 0, np.log(mass * p / np.where(tot > 0, tot, 1.0)), -np.inf).astype(np.float32)
        fin = np.where(accepting, np.log(0.1 + 0.4 * rng.random(accepting.shape)), -np.inf).astype(np.float32)
    return arc, fin


def trie(n_strings=1000, max_len=8, seed=13, alphabet=b"0123456789abyesno"):
    """(delta, accepting, start, strings, depth): the trie of seeded byte strings of 1 .. max_len bytes over the alphabet of
    `dfa_ref.synth_vocab`'s tokens."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(alphabet, np.uint8)
    strings = set()
    while len(strings) < n_strings:  # one in five short (1 .. 3 bytes: accepting inner states), the rest from half max_len up
        n = int(rng.integers(1, 4)) if rng.random() < 0.2 else int(rng.integers(max_len // 2, max_len + 1))
        strings.add(bytes(rng.choice(letters, n)))
    strings = sorted(strings)
    rows, acc = [np.full(256, -1, np.int32)], [False]
    for s in strings:
        cur = 0
        for b in s:
            if rows[cur][b] < 0:
                rows[cur][b] = len(rows)
                rows.append(np.full(256, -1, np.int32))
                acc.append(False)
            cur = int(rows[cur][b])
        acc[cur] = True
    return np.stack(rows), np.array(acc, np.bool_), 0, strings, max(map(len, strings))


def accepted_strings(delta, accepting, start, seed, n=20, max_len=3):
    """Up to n seeded byte strings the automaton accepts (random walks that stop in accepting states).  Short ones: a path
    weight is a float32 chain, every link rounded to half an ulp of a sum near -6 a byte, and the tests compare two such
    chains within 1e-5 - a few bytes keep the sums below 32, where an ulp is 1.9e-6."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(50 * n):
        s, data = int(start), []
        for _ in range(int(rng.integers(0, max_len + 1))):
            nxt = np.nonzero(delta[s] >= 0)[0]
            if len(nxt) == 0:
                break
            b = int(rng.choice(nxt))
            data.append(b)
            s = int(delta[s, b])
        if accepting[s]:
            out.append(bytes(data))
        if len(out) == n:
            break
    return out
