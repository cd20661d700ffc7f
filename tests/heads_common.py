"""Shared by the word-structure head tests and tests/golden/make_golden_heads.py: an fp64 closed form of the two target
functions (reference fft_lm/phase_clock.py:68-115, fft_lm/segmentation_head.py:58-99), written from their definition and
not from either implementation, the stub backbone of the model fixtures, and the byte patterns of the target tests.
Nothing here imports the package under test or the reference."""
import math

import numpy as np
import torch
import torch.nn as nn


def in_phase_set(v):
    """P: space and the punctuation 33..47, 58..64 -- where the phase clock breaks words."""
    return ((v >= 32) & (v <= 47)) | ((v >= 58) & (v <= 64))


def in_boundary_set(v):
    """S = P plus brackets 91..96, braces 123..126 and the newlines 10, 13 -- what ends a word for the label."""
    return in_phase_set(v) | ((v >= 91) & (v <= 96)) | ((v >= 123) & (v <= 126)) | (v == 10) | (v == 13)


def phase_closed_form(tokens):
    """(B, T) integers -> (B, T, 2) float64: position q of a maximal run of n non-P values gets (cos, sin)(pi q / (n - 1))
    (n = 1: (1, 0)), a value of P gets (0, 0).  Word starts and delimiters are exact."""
    v = np.asarray(tokens).astype(np.int64)
    B, T = v.shape
    out = np.zeros((B, T, 2), np.float64)
    for b in range(B):
        word = ~in_phase_set(v[b])
        edge = np.diff(np.concatenate(([0], word.astype(np.int8), [0])))
        for s, e in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)):
            n = int(e - s)
            ang = np.zeros(1) if n == 1 else math.pi * np.arange(n, dtype=np.float64) / (n - 1)
            out[b, s:e, 0] = np.cos(ang)
            out[b, s:e, 1] = np.sin(ang)
            out[b, s] = (1.0, 0.0)
    return out


def boundary_closed_form(tokens):
    """(B, T) integers -> (B, T) float64: 1 where value t + 1 is in S, and at t = T - 1."""
    v = np.asarray(tokens).astype(np.int64)
    out = np.ones(v.shape, np.float64)
    out[:, :-1] = in_boundary_set(v[:, 1:])
    return out


def thread_run(T):
    """Positions one thread of k_word_targets owns (csrc/smx_ema.hip): 256 threads a row, each a contiguous run of
    ceil(ceil(T / 64) / 256) words of 64 positions.  64 up to T = 16384."""
    words = -(-T // 64)
    return 64 * -(-words // 256)


WORD, SPACE = 97, 32


def _words(B, T, n, first_is_word):
    """rows of n word bytes then one delimiter, repeated; row b is shifted by b so that the rows differ"""
    t = np.arange(T)[None, :] + np.arange(B)[:, None] + (0 if first_is_word else n)
    return np.where(t % (n + 1) < n, WORD, SPACE).astype(np.int64)


def patterns(B, T, seed=0):
    """name -> (B, T) int64 byte rows."""
    g = np.random.default_rng(seed + 1000 * B + T)
    out = {"uniform": g.integers(0, 256, (B, T)),
           "one_word": g.integers(97, 123, (B, T)),                       # one word of length T
           "all_delims": g.choice(np.array([32, 33, 47, 58, 64]), (B, T)),
           "alternating": _words(B, T, 1, True),                          # words of length 1
           "alternating_delim_first": _words(B, T, 1, False),
           "words_of_2": _words(B, T, 2, True)}
    inside = _words(B, T, 5, True)
    inside[:, 0] = inside[:, -1] = WORD                                    # starts and ends inside a word
    if T > 1:
        inside[:, 1] = inside[:, -2] = WORD
    out["ends_inside_words"] = inside
    on = _words(B, T, 5, True)
    on[:, 0] = on[:, -1] = SPACE                                           # starts and ends on a delimiter
    out["ends_on_delims"] = on
    run = thread_run(T)
    for off in (-1, 0, 1):                                                 # a delimiter at, before and after every run edge
        x = g.integers(97, 123, (B, T))
        pos = np.arange(0, T + run, run) + off
        x[:, pos[(pos >= 0) & (pos < T)]] = SPACE
        out["run_edge_%+d" % off] = x
    mixed = np.concatenate(([10, 13], np.arange(91, 97), np.arange(123, 127), np.arange(128, 256, 9), [97, 98, 32, 46]))
    out["sets_disagree"] = g.choice(mixed, (B, T))                         # 10, 13, 91-96, 123-126, bytes >= 128
    return {k: np.ascontiguousarray(v, dtype=np.int64) for k, v in out.items()}


def wide_values(B, T, seed=0):
    """int64 storage only: values outside 0..255 (word bytes: the reference compares numbers) among delimiters."""
    g = np.random.default_rng(seed + 7)
    return g.choice(np.array([-1, -32, 256 + 32, 300, (1 << 40) + 32, 32, 46, 97, 10 + 256]), (B, T)).astype(np.int64)


EDGE_ROWS = ["The cat sat.", " leading and trailing ", "a", " ", "a b", "ab", "x\ny\rz[w]{v}~u", "end.", "...",
             "one-two:three;four@five"]


def edge_rows():
    """The short rows of the targets fixture, space-padded to one width: (B, 24) int64."""
    w = max(len(r) for r in EDGE_ROWS)
    return np.array([[ord(c) for c in r.ljust(w)] for r in EDGE_ROWS], np.int64)


class _Cfg:
    def __init__(self, d_model):
        self.d_model = d_model


class StubBackbone(nn.Module):
    """The smallest backbone the word-structure models accept: `cfg.d_model` and forward_hidden = embedding + Linear.
    The hidden states of the last call are kept (with their gradient) for the tests."""

    def __init__(self, d_model=32):
        super().__init__()
        self.cfg = _Cfg(d_model)
        self.embed = nn.Embedding(256, d_model)
        self.mix = nn.Linear(d_model, d_model)
        self.last_hidden = None

    def forward_hidden(self, x, cutoff=None):
        h = self.mix(self.embed(x.long()))
        if h.requires_grad:
            h.retain_grad()
        self.last_hidden = h
        return h


def t(a, device=None):
    out = torch.from_numpy(np.ascontiguousarray(a))
    return out if device is None else out.to(device)
