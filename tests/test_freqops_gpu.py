"""The native frequency attention and frequency layernorm (csrc/smx_freq.hip) and what stands on them, on the GPU.

Yardstick of every case: the formulas of tests/freqops_common.py on complex128 copies on the CPU; bound TOL_ACT = 1e-5
max-normalised (the reference's own fp32 error over these shapes: 1.1e-7 .. 3.0e-7 attention, 1.2e-7 .. 1.0e-6
layernorm), except the overflow case, whose bound max(TOL_ACT, 4 e_ref) is worked out there.  Every case prints its
error before it asserts; the measured values are in DESIGN 7o."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import TOL_ACT, load_golden, rel_err

import freqops_common as fc

pytestmark = pytest.mark.gpu

ATTN_SHAPES = [(2, 2, 8, 4), (2, 4, 64, 1), (1, 3, 65, 3), (2, 2, 1025, 5), (1, 2, 5000, 64),
               (1, 2, 9, 131),        # 66 pairs a row: more than one 64-lane pass, the row cut at both ends
               (1, 40, 3300, 2)]      # 2080 tiles of 64 rows: past the 2048 workgroups at which the tiles double
LN_SHAPES = [(2, 8, 4), (3, 5, 2), (2, 7, 3), (4, 33, 64), (2, 9, 130), (1, 3, 1000),
             (2, 3, 300),             # Vec<4> x 4
             (2, 3, 131), (1, 2, 1023),   # Vec<2> x 4 and x 16
             (1, 2, 1024),            # the widest in-register row
             (1, 2, 1025), (1, 2, 1026),  # one past it, odd and even: the torch composition
             # every instance at the width that fills it and at the first one past its smaller neighbour
             (1, 2, 128), (1, 2, 256), (1, 2, 258), (1, 2, 512), (1, 2, 514),
             (1, 2, 63), (1, 2, 65), (1, 2, 255), (1, 2, 257),
             (3, 3000, 4)]            # 9000 rows: more than the 8192 wavefronts of the grid, a wavefront walks two rows


def _inputs(seed, *shapes):
    gen = torch.Generator().manual_seed(seed)
    return [fc.crandn(gen, *s) for s in shapes]


def _err(got, want, what):
    e = rel_err(got.detach().cpu().resolve_conj().numpy(), want.resolve_conj().numpy())
    print(f"{what}: rel_err {e:.3g}")
    return e


@pytest.fixture(scope="module")
def attn_cases():
    """inputs and complex128 results per (shape, temperature), computed once"""
    memo = {}

    def get(shape, temperature):
        key = (shape, temperature)
        if key not in memo:
            q, k, v = _inputs(11, shape, shape, shape)
            memo[key] = (q, k, v, fc.attention_ref(fc.wide(q), fc.wide(k), fc.wide(v), temperature))
        return memo[key]
    return get


@pytest.mark.parametrize("temperature", [1.0, 0.5])
@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention(gpu, attn_cases, shape, temperature):
    import tensor_cuda_fft_amd as pkg
    q, k, v, want = attn_cases(shape, temperature)
    out = pkg.FrequencyAttention.frequency_attention(q.to(gpu), k.to(gpu), v.to(gpu), temperature)
    assert out.shape == shape and out.is_contiguous() and out.dtype == torch.complex64
    assert _err(out, want, f"attention {shape} T={temperature}") <= TOL_ACT


@pytest.mark.parametrize("temperature", [1.0, 0.5])
@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_head_transposed_views(gpu, attn_cases, shape, temperature):
    """(B, N, H, hd) tensors read as (B, H, N, hd) views; merge_heads writes (B, N, H hd) directly"""
    from tensor_cuda_fft_amd import functional as fn
    q, k, v, want = attn_cases(shape, temperature)
    views = [t.permute(0, 2, 1, 3).contiguous().to(gpu).permute(0, 2, 1, 3) for t in (q, k, v)]
    assert shape[1] == 1 or shape[2] == 1 or not views[0].is_contiguous()
    out = fn.frequency_attention(*views, temperature)
    assert _err(out, want, f"views {shape}") <= TOL_ACT
    merged = fn.frequency_attention(*views, temperature, merge_heads=True)
    B, H, N, D = shape
    assert merged.shape == (B, N, H * D) and merged.is_contiguous()
    assert _err(merged, fc.merge_heads(want), f"views merged {shape}") <= TOL_ACT


def test_attention_strides_and_alignment(gpu):
    """a non-unit innermost stride (copied by the glue); rows 8 bytes off a 16-byte boundary on one side only (q against
    k, v against out: the element-by-element walk); rows that alternate between both alignments (odd row stride)"""
    from tensor_cuda_fft_amd import functional as fn
    B, H, N, D = 2, 2, 9, 6
    q, k, v = _inputs(12, (B, H, N, D), (B, H, N, D), (B, H, N, D))
    want = fc.attention_ref(fc.wide(q), fc.wide(k), fc.wide(v))
    wide_q = torch.zeros(B, H, N, 2 * D, dtype=torch.complex64, device=gpu)
    wide_q[..., ::2] = q.to(gpu)
    assert _err(fn.frequency_attention(wide_q[..., ::2], k.to(gpu), v.to(gpu)), want, "innermost stride 2") <= TOL_ACT
    for who in ("q", "k", "v"):
        ops = {"q": q.to(gpu), "k": k.to(gpu), "v": v.to(gpu)}
        pad = torch.zeros(B, H, N, D + 1, dtype=torch.complex64, device=gpu)      # row stride 7: alignments alternate
        pad[..., 1:] = ops[who]
        ops[who] = pad[..., 1:]
        assert ops[who].stride(-1) == 1 and ops[who].data_ptr() % 16 == 8
        assert _err(fn.frequency_attention(ops["q"], ops["k"], ops["v"]), want, f"{who} off by 8 bytes") <= TOL_ACT


def test_attention_small_and_empty(gpu):
    from tensor_cuda_fft_amd import functional as fn
    q, k, v = _inputs(13, (2, 3, 1, 5), (2, 3, 1, 5), (2, 3, 1, 5))
    out = fn.frequency_attention(q.to(gpu), k.to(gpu), v.to(gpu))
    assert _err(out, fc.wide(v), "N = 1: p = 1") <= 1e-7
    e = torch.empty(0, 2, 4, 3, dtype=torch.complex64, device=gpu)
    assert fn.frequency_attention(e, e, e).shape == (0, 2, 4, 3)
    assert fn.frequency_attention(e, e, e, merge_heads=True).shape == (0, 4, 6)
    # a temperature that is 0 or inf as the C entry's float takes the torch ops, as the reference would: no SmxError
    q, k, v = (t.to(gpu) for t in (q, k, v))
    assert fn.frequency_attention(q, k, v, 1e-50).shape == q.shape
    assert _err(fn.frequency_attention(q, k, v, 1e39), fc.wide(v), "N = 1, T = 1e39") <= 1e-7


def test_attention_scores_near_100_do_not_overflow(gpu):
    """|q| = |k| ~ 10 (1 + 0.01 randn), random phases: scores near 100, exp(100) is beyond fp32 without the max
    subtraction.  Bound max(TOL_ACT, 4 e_ref), e_ref the error of the complex64 formulas on the CPU at the same inputs
    (measured 5.5e-6 .. 7.4e-6 over three seeds; 5.2e-6 on this one, the kernel 6.2e-6 on one MI355X): a score near 100
    carries a rounding of ~1 ulp = 7.6e-6 that exp turns into a relative error of that size, and another summation order
    moves it by a small multiple."""
    from tensor_cuda_fft_amd import functional as fn
    gen = torch.Generator().manual_seed(14)
    shape = (1, 2, 300, 5)

    def big():
        mag = 10 * (1 + 0.01 * torch.randn(*shape, generator=gen))
        return torch.polar(mag, 6.2831853 * torch.rand(*shape, generator=gen))
    q, k, v = big(), big(), fc.crandn(gen, *shape)
    want = fc.attention_ref(fc.wide(q), fc.wide(k), fc.wide(v))
    e_ref = rel_err(fc.attention_ref(q, k, v).numpy(), want.numpy())
    out = fn.frequency_attention(q.to(gpu), k.to(gpu), v.to(gpu))
    assert bool(torch.isfinite(torch.view_as_real(out)).all())
    print(f"e_ref {e_ref:.3g}")
    assert _err(out, want, "scores near 100") <= max(TOL_ACT, 4 * e_ref)


@pytest.fixture(scope="module")
def ln_cases():
    memo = {}

    def get(shape):
        if shape not in memo:
            z, = _inputs(21, shape)
            z[..., 0, shape[-1] // 2] = 0                    # exact zeros in the first row of every batch entry
            memo[shape] = z
        return memo[shape]
    return get


@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layernorm(gpu, ln_cases, shape):
    import tensor_cuda_fft_amd as pkg
    z = ln_cases(shape)
    out = pkg.frequency_layernorm(z.to(gpu))
    assert out.shape == shape and out.is_contiguous()
    assert _err(out, fc.layernorm_ref(fc.wide(z)), f"layernorm {shape}") <= TOL_ACT
    mid = shape[-1] // 2
    assert bool((out[..., 0, mid].imag == 0).all())            # the phase of an exact zero is 0


def test_layernorm_eps_views_and_width_one(gpu, ln_cases):
    import tensor_cuda_fft_amd as pkg
    z = ln_cases((4, 33, 64))
    out = pkg.frequency_layernorm(z.to(gpu), eps=0.25)
    assert _err(out, fc.layernorm_ref(fc.wide(z), 0.25), "eps = 0.25") <= TOL_ACT
    zt = z.to(gpu).transpose(0, 1)                           # a non-contiguous input
    assert _err(pkg.frequency_layernorm(zt), fc.layernorm_ref(fc.wide(z)).transpose(0, 1), "transposed") <= TOL_ACT
    one = pkg.frequency_layernorm(torch.ones(5, 1, dtype=torch.complex64, device=gpu))
    assert bool(torch.isnan(torch.view_as_real(one)).all())  # D = 1: NaN, as the reference
    assert pkg.frequency_layernorm(torch.empty(0, 4, dtype=torch.complex64, device=gpu)).shape == (0, 4)


@pytest.mark.parametrize("name", ["U06_flayer_2x33x64_h4", "U07_flayer_1x5x6_h3"])
def test_layer_equals_the_reference(gpu, name):
    import tensor_cuda_fft_amd as pkg
    g = load_golden(name)
    x = torch.from_numpy(g["x"]).to(gpu)
    layer = pkg.FrequencyTransformerLayer(x.shape[-1], int(g["heads"]), device=gpu)
    assert layer.q_proj_freq.is_cuda and layer.q_proj_freq.dtype == torch.complex64
    for attr in ("q_proj_freq", "k_proj_freq", "v_proj_freq", "o_proj_freq"):
        setattr(layer, attr, torch.from_numpy(g["w" + attr[0]]).to(gpu))
    out = layer.forward(x)
    assert out.shape == x.shape and out.is_contiguous()
    assert _err(out, torch.from_numpy(g["out"]), name) <= TOL_ACT
    layer.o_proj_freq = layer.o_proj_freq * 2                # reassigned between calls
    assert _err(layer.forward(x), torch.from_numpy(2 * g["out"]), name + " reassigned") <= TOL_ACT


def test_golden_ops_on_the_device(gpu):
    """the small members on the device: attention and layernorm goldens, the embedding with an injected table, and
    circulant_matmul through the package's own transform"""
    import tensor_cuda_fft_amd as pkg
    g = load_golden("U02_fattn_1x3x65x3_t05")
    q, k, v = (torch.from_numpy(g[n]).to(gpu) for n in "qkv")
    out = pkg.FrequencyAttention.frequency_attention(q, k, v, float(g["temperature"]))
    assert _err(out, torch.from_numpy(g["out"]), "U02") <= TOL_ACT
    g = load_golden("U04_fln_2x7x3_zeros")
    z = torch.from_numpy(g["z"]).to(gpu)
    assert _err(pkg.frequency_layernorm(z, float(g["eps"])), torch.from_numpy(g["out"]), "U04") <= TOL_ACT
    assert _err(pkg.frequency_relu(z), torch.from_numpy(g["relu"]), "U04 relu") <= TOL_ACT
    g = load_golden("U08_embedding_50x16")
    emb = pkg.ComplexSemanticEmbedding(50, 16, device=gpu)
    assert emb.freq_embeddings.is_cuda and emb.freq_embeddings.shape == (50, 16)
    assert 0 < float(emb.freq_embeddings.abs().max()) < 0.2
    emb.freq_embeddings = torch.from_numpy(g["freq_embeddings"]).to(gpu)
    e = emb.lookup(torch.from_numpy(g["ids"]).to(gpu))
    assert _err(e, torch.from_numpy(g["lookup"]), "lookup") == 0
    assert _err(emb.semantic_similarity(e[0], e[1]), torch.from_numpy(g["similarity"]), "similarity") <= TOL_ACT
    assert _err(emb.phase_relationship(e[0], e[1]), torch.from_numpy(g["phase"]), "phase") <= TOL_ACT
    g = load_golden("U09_circulant_2x5x12x20")
    x = torch.from_numpy(g["x"]).to(gpu)
    for w, o in (("w_out_in", "out_out_in"), ("w_k_n", "out_k_n")):
        y = pkg.FrequencyMatMul.circulant_matmul(x, torch.from_numpy(g[w]).to(gpu))
        assert _err(y, torch.from_numpy(g[o]), "circulant " + w) <= TOL_ACT
    with pytest.raises(ValueError, match="Dimension mismatch: x has 12"):
        pkg.FrequencyMatMul.circulant_matmul(x, torch.zeros(7, 9, dtype=torch.complex64, device=gpu))


def test_inputs_that_require_grad_take_the_composition(gpu):
    import tensor_cuda_fft_amd as pkg
    q, k, v, go = _inputs(31, *[(2, 2, 6, 3)] * 4)
    leaves = [t.to(gpu).requires_grad_(True) for t in (q, k, v)]
    got = torch.autograd.grad(pkg.FrequencyAttention.frequency_attention(*leaves, 0.7), leaves, go.to(gpu))
    wide = [fc.wide(t).requires_grad_(True) for t in (q, k, v)]
    want = torch.autograd.grad(fc.attention_ref(*wide, 0.7), wide, fc.wide(go))
    for a, b, n in zip(got, want, "qkv"):
        assert _err(a, b, "grad_" + n) <= TOL_ACT
    z, gz = _inputs(32, (3, 5, 6), (3, 5, 6))
    leaf = z.to(gpu).requires_grad_(True)
    got, = torch.autograd.grad(pkg.frequency_layernorm(leaf), leaf, gz.to(gpu))
    wz = fc.wide(z).requires_grad_(True)
    want, = torch.autograd.grad(fc.layernorm_ref(wz), wz, fc.wide(gz))
    assert _err(got, want, "grad_z") <= TOL_ACT
    with torch.no_grad():                                    # grad mode off: the native path, same values
        out = pkg.frequency_layernorm(leaf)
    assert not out.requires_grad and _err(out, fc.layernorm_ref(fc.wide(z)), "no_grad") <= TOL_ACT


def test_two_runs_and_a_graph_replay_are_bitwise_equal(gpu):
    from tensor_cuda_fft_amd import functional as fn
    q, k, v = (t.to(gpu) for t in _inputs(41, *[(2, 3, 1025, 5)] * 3))
    z = _inputs(42, (4, 33, 130))[0].to(gpu)

    def step():
        return fn.frequency_attention(q, k, v, 0.5), fn.frequency_attention(q, k, v, merge_heads=True), \
            fn.frequency_layernorm(z)
    first = [t.clone() for t in step()]                      # (eager once before the capture: INTEGRATION.md)
    for a, b in zip(step(), first):
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, first):
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def test_raw_entries_refuse_bad_arguments(gpu):
    """NULL pointers, negative sizes, a short or missing workspace: SMX_ERR_INVALID and nothing enqueued (the output
    keeps its fill); zero-sized problems succeed without touching anything"""
    from tensor_cuda_fft_amd import _lib
    lib = _lib.lib()
    B, H, N, D = 1, 2, 8, 4
    q, k, v = (t.to(gpu) for t in _inputs(51, *[(B, H, N, D)] * 3))
    out = torch.full((B, H, N, D), 7.0, dtype=torch.complex64, device=gpu)
    need = ctypes.c_size_t()
    assert lib.smx_freq_attention_workspace_bytes(B, H, N, ctypes.byref(need)) == 0
    assert need.value == 65536 + 256                         # the reserved header, then B H N floats rounded to 256
    assert lib.smx_freq_attention_workspace_bytes(B, H, N, None) == _lib.SMX_ERR_INVALID
    assert lib.smx_freq_attention_workspace_bytes(-1, H, N, ctypes.byref(need)) == _lib.SMX_ERR_INVALID
    ws = torch.empty(65536 + 256, dtype=torch.uint8, device=gpu)
    st = (H * N * D, N * D, D)
    stream = torch.cuda.current_stream().cuda_stream

    def call(qp=q.data_ptr(), op=out.data_ptr(), wsp=ws.data_ptr(), wsn=ws.numel(), b=B, d=D, temp=1.0, stride=st):
        return lib.smx_freq_attention_forward(qp, *stride, k.data_ptr(), *st, v.data_ptr(), *st, op, *st, temp, wsp, wsn,
                                              b, H, N, d, stream)
    for bad in (dict(qp=None), dict(op=None), dict(wsp=None), dict(wsn=ws.numel() - 1), dict(wsn=0), dict(b=-1),
                dict(d=-1), dict(temp=0.0), dict(temp=float("inf")), dict(stride=(-1, N * D, D))):
        assert call(**bad) == _lib.SMX_ERR_INVALID, bad
        assert _lib.lib().smx_last_error()
    assert call(b=0) == 0 and call(d=0) == 0 and call(b=0, qp=None, op=None, wsp=None, wsn=0) == 0
    zin = torch.ones(3, 4, dtype=torch.complex64, device=gpu)
    zout = torch.full((3, 4), 7.0, dtype=torch.complex64, device=gpu)
    ln = lib.smx_freq_layernorm_forward
    assert ln(None, zout.data_ptr(), 1e-5, 3, 4, stream) == _lib.SMX_ERR_INVALID
    assert ln(zin.data_ptr(), None, 1e-5, 3, 4, stream) == _lib.SMX_ERR_INVALID
    assert ln(zin.data_ptr(), zout.data_ptr(), 1e-5, -3, 4, stream) == _lib.SMX_ERR_INVALID
    assert ln(zin.data_ptr(), zout.data_ptr(), 1e-5, 3, 1025, stream) == _lib.SMX_ERR_UNSUPPORTED
    assert ln(zin.data_ptr(), zout.data_ptr(), 1e-5, 0, 4, stream) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((zout == 7).all())
    assert call() == 0                                       # and the same arguments, all valid, run
    torch.cuda.synchronize()
    want = fc.attention_ref(fc.wide(q), fc.wide(k), fc.wide(v))
    assert _err(out, want, "raw call") <= TOL_ACT
    assert lib.smx_version() == 303
