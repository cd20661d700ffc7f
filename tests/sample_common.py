"""The byte sampler's definition (include/smx.h, smx_sample_bytes) restated literally, row by row, in fp64 -- written from
the ten steps, not from any implementation -- and the two margins that say whether a row can be compared at all.

A row is COMPARABLE when no running sum of step 7 comes within MARGIN of top_p and no running sum of step 10 within
MARGIN of u: an fp32 sum of 256 terms is off by about 1.5e-5 at worst, so inside 1e-4 either side of the threshold is a
legitimate answer.  A test may leave out at most MAX_SKIP of its rows and asserts that (share()).

The float parameters are taken as the fp32 values the entry receives (temperature 0.8 is 0.800000012): the same function,
not a neighbour of it.
"""
import math

import numpy as np

MARGIN = 1e-4
MAX_SKIP = 0.10
NINF = -math.inf


def _f32(v):
    return float(np.float32(v))


def restate_row(logits, recent, u, *, temperature=1.0, top_p=1.0, top_k=0, repetition_penalty=1.0, presence_penalty=0.0,
                frequency_penalty=0.0, ascii_only=False, ban_cr=False, max_run_length=0):
    """One row: (id, p (256) fp64, margin of step 7 (inf where the step is skipped), margin of step 10)."""
    temperature, top_p, rep = _f32(temperature), _f32(top_p), _f32(repetition_penalty)
    pres, freq = _f32(presence_penalty), _f32(frequency_penalty)
    l = [float(v) for v in np.asarray(logits, np.float64)]                               # 1
    assert len(l) == 256
    recent = [int(b) for b in recent]
    count = {}
    for b in recent:
        if 0 <= b < 256:
            count[b] = count.get(b, 0) + 1
    for b in count:                                                                      # 2
        l[b] = l[b] / rep
    if pres != 0.0 or freq != 0.0:                                                       # 3
        for b, c in count.items():
            l[b] = l[b] - (pres + freq * c)
    if ascii_only:                                                                       # 4
        for b in range(256):
            if not (b == 10 or 32 <= b <= 126):
                l[b] = NINF
    if ban_cr:
        l[13] = NINF
    if max_run_length > 0 and len(recent) >= max_run_length:                             # 5
        tail = recent[len(recent) - max_run_length:]
        if all(b == tail[-1] for b in tail) and 0 <= tail[-1] < 256:
            l[tail[-1]] = NINF
    l = [v / temperature for v in l]                                                     # 6
    margin_p = math.inf
    if top_p < 1.0:                                                                      # 7
        order = sorted(range(256), key=lambda j: (-l[j], j))
        m = l[order[0]]
        e = [math.exp(l[j] - m) for j in order]
        s = math.fsum(e)
        run, kept = 0.0, 0
        for i in range(256):
            run += e[i] / s
            margin_p = min(margin_p, abs(run - top_p))
            if run <= top_p:
                kept = i + 1
        kept = max(kept, 1)
        for j in order[kept:]:
            l[j] = NINF
    if top_k > 0:                                                                        # 8
        v = sorted(l, reverse=True)[min(top_k, 256) - 1]
        l = [NINF if x < v else x for x in l]
    m = max(l)                                                                           # 9
    e = [math.exp(x - m) for x in l]
    s = math.fsum(e)
    p = [x / s for x in e]
    u = float(u)                                                                         # 10
    run, pick, margin_u = 0.0, None, math.inf
    for j in range(256):
        run += p[j]
        margin_u = min(margin_u, abs(run - u))
        if pick is None and run > u:
            pick = j
    if pick is None:
        pick = max(j for j in range(256) if p[j] > 0)
    return pick, np.array(p, np.float64), margin_p, margin_u


def restate(logits, recent, u, **kw):
    """Rows (R, 256), the shared window, u (R) -> ids (R) int64, probs (R, 256) fp64, comparable (R) bool."""
    logits, u = np.asarray(logits), np.asarray(u)
    rows = [restate_row(logits[r], recent, u[r], **kw) for r in range(logits.shape[0])]
    ids = np.array([r[0] for r in rows], np.int64)
    probs = np.stack([r[1] for r in rows])
    ok = np.array([r[2] > MARGIN and r[3] > MARGIN for r in rows])
    return ids, probs, ok


def share(ok):
    """The part of the rows left out; a test asserts it is at most MAX_SKIP."""
    return 1.0 - float(np.mean(ok))


def banned(ascii_only=False, ban_cr=False, **_):
    """The bytes steps 4 can never let through, as a (256) bool array."""
    b = np.zeros(256, bool)
    if ascii_only:
        b[:] = True
        b[10] = False
        b[32:127] = False
    if ban_cr:
        b[13] = True
    return b


# the settings the tests walk: every switch on its own, and all together
SETTINGS = {
    "plain": dict(),
    "temperature": dict(temperature=0.8),
    "top_p": dict(temperature=0.8, top_p=0.9),
    "top_p_half": dict(temperature=0.8, top_p=0.5),
    "top_k": dict(temperature=0.8, top_k=5),
    "repetition": dict(temperature=0.8, repetition_penalty=1.25),
    "presence_frequency": dict(temperature=0.8, presence_penalty=0.3, frequency_penalty=0.05),
    "ascii_only": dict(temperature=0.8, ascii_only=True),
    "ban_cr": dict(temperature=0.8, ban_cr=True),
    "max_run": dict(temperature=0.8, max_run_length=6),
    "all": dict(temperature=0.8, top_p=0.9, top_k=40, repetition_penalty=1.25, presence_penalty=0.3,
                frequency_penalty=0.05, ascii_only=True, ban_cr=True, max_run_length=6),
}


def make_rows(R, seed, scale=3.0):
    """(logits (R, 256) fp32 = scale * randn, u (R) fp32 in [0, 1)) from a fixed seed."""
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((R, 256))).astype(np.float32), rng.random(R, dtype=np.float32)


def make_window(n, seed, run=0):
    """n ids in 0..255 drawn mostly from lower-case text bytes (so that bytes repeat); the last `run` are one byte."""
    rng = np.random.default_rng(seed)
    w = rng.choice(np.array([32, 10, 13, 101, 116, 97, 111, 200] + list(range(97, 123))), n).astype(np.int64)
    if run:
        w[n - run:] = 101
    return w
