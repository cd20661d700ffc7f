"""The epoch-end pieces on the GPU: the native multi-pattern byte search (csrc/smx_match.hip) against bytes.find on the
host copy -- every tile edge, corpus alignment, snippet shape and workgroup count the kernel treats differently --, its
reproducibility and graph capture, and parroting_score / eval_loss against the reference's recorded results (V01, V02)."""
import numpy as np
import pytest
import torch

import eval_common as ec
from conftest import TOL_ACT, load_golden, rel_err
from eval_common import TILE

pytestmark = pytest.mark.gpu


def pkg():
    import tensor_cuda_fft_amd
    return tensor_cuda_fft_amd


def check(corpus: torch.Tensor, snips: torch.Tensor, dev, view=None, **kw):
    """find_snippets on the device equals bytes.find on the host copy, exactly; returns the answers.  `view`: the
    device tensor to search when it is not simply corpus.to(dev)."""
    want = ec.find_all(bytes(corpus.tolist()), snips)
    got = pkg().find_snippets(corpus.to(dev) if view is None else view, snips.to(dev), **kw)
    assert got.dtype == torch.int64 and got.device.type == "cuda" and got.shape == want.shape
    assert torch.equal(got.cpu(), want), (corpus.numel(), tuple(snips.shape), kw, got.cpu().tolist(), want.tolist())
    return want


@pytest.mark.parametrize("L", [4, 5, 64, 255, 256])
def test_find_snippets_at_every_tile_edge(gpu, L):
    """n below, at and above a snippet, inside one tile, at a tile's last position, with the halo just reaching into the
    next tile, and over three tiles and a bit; snippets at 0, at n - L, across every tile boundary by 1, L / 2 and L - 1
    bytes, cut off by the end, duplicated, and sharing their first four bytes."""
    seen = set()
    for n in (L - 1, L, L + 1, 1000, TILE, TILE + L - 2, TILE + L - 1, TILE + L, 3 * TILE + 5):
        corpus, snips = ec.planted_case(n, L, 23, 100 + n % 97 + L)
        want = check(corpus, snips, gpu)
        seen |= set(want.tolist())
        if n >= L:
            assert want[0] == 0 and want[2] == 0 and want[4] == -1 and (L == 4 or want[3] == -1)
        if n == 3 * TILE + 5:
            assert {TILE - 1, TILE - L // 2, TILE - (L - 1), 2 * TILE - 1, n - L} <= set(want.tolist())
    assert -1 in seen and len(seen) > 8


@pytest.mark.parametrize("S", [1, 256])
def test_find_snippets_one_and_256_snippets(gpu, S):
    corpus, snips = ec.planted_case(2 * TILE + 100, 64, S, 5 + S)
    want = check(corpus, snips, gpu)
    assert want[0] == 0 and (S == 1 or ((want >= 0).sum() >= 8 and (want < 0).sum() >= 200))


def test_find_snippets_in_a_corpus_of_one_repeated_byte(gpu):
    L, n = 64, 2 * TILE + 77
    corpus = torch.full((n,), 32, dtype=torch.uint8)
    yes = torch.full((L,), 32, dtype=torch.uint8)
    no = yes.clone()
    no[-1] = ord("x")                                            # matches 63 bytes at every position, never 64
    late = no.clone()
    corpus[n - 1] = ord("x")                                     # ... until the corpus ends in it
    want = check(corpus, torch.stack([yes, no, late, yes]), gpu)
    assert want.tolist() == [0, n - L, n - L, 0]
    corpus[n - 1] = 32
    assert check(corpus, torch.stack([yes, no]), gpu).tolist() == [0, -1]


@pytest.mark.parametrize("offset", [1, 7, 15])
def test_find_snippets_reads_a_misaligned_view_in_place_and_nothing_outside_it(gpu, offset):
    """The corpus is bytes [offset, offset + n) of a larger allocation, n no multiple of 16.  Snippets that begin before
    the view or end after it are in the allocation but not in the corpus: an answer other than -1 is a read outside."""
    L, n, pad = 64, 2 * TILE + 101, 256
    corpus, snips = ec.planted_case(n, L, 40, 31 + offset, phase=offset)
    big = ec.random_corpus(pad + n + pad, 77 + offset, 0, 200)
    big[pad + offset:pad + offset + n] = corpus
    lo, hi = pad + offset, pad + offset + n
    outside = torch.stack([big[lo - 3:lo - 3 + L], big[lo - L + 1:lo + 1], big[hi - L + 2:hi + 2], big[hi - 1:hi - 1 + L]])
    snips = torch.cat([snips[:36], outside])
    dbig = big.to(gpu)
    view = dbig[lo:hi]
    assert view.data_ptr() % 16 == offset and n % 16 != 0
    want = check(corpus, snips, gpu, view=view)
    assert want[36:].tolist() == [-1] * 4 and want[0] == 0 and want[1] == n - L
    edge = TILE - offset                                         # the first position of the scan's second tile
    assert {edge - 1, edge - L // 2, edge - (L - 1), edge + TILE - 1} <= set(want.tolist())
    strided = dbig[::2]                                          # non-contiguous: made contiguous
    assert torch.equal(pkg().find_snippets(strided, snips.to(gpu)).cpu(), ec.find_all(bytes(big[::2].tolist()), snips))


@pytest.mark.parametrize("max_workgroups", [1, 2, 0])
def test_find_snippets_multi_tile_walk(gpu, max_workgroups):
    """five tiles walked by one workgroup, by two (three and two tiles) and by five"""
    corpus, snips = ec.planted_case(5 * TILE - 100, 64, 23, 9)
    want = check(corpus, snips, gpu, max_workgroups=max_workgroups)
    assert {t * TILE - 1 for t in (1, 2, 3, 4)} <= set(want.tolist())


def test_find_snippets_joins_more_than_256_table_rows(gpu):
    """257 tiles and a bit under the default workgroup count: one workgroup per tile, so the (G, S) table has more rows
    than k_match_join has threads and thread j takes rows j and j + 256.  The snippet planted at n - L begins in the last
    tile (row 257 of the table) and, being found there first, nowhere else: its answer comes through the second step."""
    L = 64
    n = 257 * TILE + 100
    corpus, snips = ec.planted_case(n, L, 23, 12)
    want = check(corpus, snips, gpu)
    assert (n - L + 1 + TILE - 1) // TILE > 256 and (n - L) // TILE >= 256
    assert want[1] == n - L                                      # bytes.find's FIRST occurrence is the last position
    assert want[0] == 0 and want[3] == -1 and want[4] == -1       # ... and absent ones stay absent over all the rows
    assert {t * TILE - 1 for t in (1, 2, 3, 4, 5, 6)} <= set(want.tolist())


def test_find_snippets_is_bitwise_reproducible(gpu):
    corpus, snips = ec.planted_case(4 * TILE + 9, 64, 64, 3)
    c, s = corpus.to(gpu), snips.to(gpu)
    a, b = pkg().find_snippets(c, s), pkg().find_snippets(c, s)
    assert torch.equal(a, b) and torch.equal(a.cpu(), ec.find_all(bytes(corpus.tolist()), snips))


def test_find_snippets_unsupported_sets_take_the_host_route(gpu):
    corpus = ec.random_corpus(5000, 2, 0, 200)
    for L in (3, 300):                                           # outside smx_match_supported
        snips = torch.stack([corpus[10:10 + L], corpus[5000 - L:], torch.full((L,), 250, dtype=torch.uint8)])
        check(corpus, snips, gpu)


def test_find_snippets_is_captured_in_a_graph_and_follows_the_corpus(gpu):
    """No host synchronisation and no allocation in the op: one captured call, replayed over new corpus contents."""
    p = pkg()
    n, L = 2 * TILE + 50, 64
    first, snips = ec.planted_case(n, L, 23, 41)
    second = ec.random_corpus(n, 43, 0, 200)
    second[TILE - 7:TILE - 7 + L] = snips[5]                      # the new contents hold snippet 5 across the tile edge
    second[300:300 + L] = snips[1]
    buf, s = first.to(gpu), snips.to(gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        p.find_snippets(buf, s)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = p.find_snippets(buf, s)
    graph.replay()
    torch.cuda.synchronize()
    want_first = ec.find_all(bytes(first.tolist()), snips)
    assert torch.equal(out.cpu(), want_first)
    buf.copy_(second.to(gpu))
    graph.replay()
    torch.cuda.synchronize()
    want_second = ec.find_all(bytes(second.tolist()), snips)
    assert torch.equal(out.cpu(), want_second) and not torch.equal(want_first, want_second)
    assert want_second[5] == TILE - 7 and want_second[1] == 300


def test_parroting_score_with_the_corpus_on_the_device(gpu):
    p = pkg()
    z = load_golden("V01_parroting")
    corpus = torch.from_numpy(z["corpus"].copy()).to(gpu)
    cfg = p.TrainConfig()
    for g in z["names"]:
        got = p.parroting_score(corpus, bytes(z[f"{g}.gen"].tobytes()), cfg)
        assert isinstance(got, float) and got == float(z[f"{g}.score"]), g


@pytest.mark.parametrize("geom", ec.GEOMETRIES)
def test_eval_loss_with_model_and_corpus_on_the_device(gpu, geom):
    p = pkg()
    z = load_golden("V02_eval_loss")
    model, cfg, starts = ec.load_lm(p, z, geom, gpu)
    corpus = torch.from_numpy(z["corpus"].copy()).to(gpu)
    model.train()
    for cname, cutoff in (("none", None), ("cut", int(z[geom + ".cutoff"]))):
        assert float(z[f"{geom}.ref_err_{cname}"]) <= TOL_ACT / 4
        torch.manual_seed(int(z["seed"]))
        got = p.eval_loss(model, corpus, starts, cfg, cutoff)
        e = rel_err(np.float64(got), z[f"{geom}.loss64.{cname}"])
        print(f"{geom} cutoff={cutoff}: loss {got!r} reference {float(z[f'{geom}.loss64.{cname}'])!r} rel_err {e:.3g}")
        assert isinstance(got, float) and e <= TOL_ACT
        assert not model.training
    torch.manual_seed(int(z["seed"]))                            # a CPU corpus beside a device model: windows are copied
    got = p.eval_loss(model, corpus.cpu(), starts, cfg, None)
    assert rel_err(np.float64(got), z[f"{geom}.loss64.none"]) <= TOL_ACT
