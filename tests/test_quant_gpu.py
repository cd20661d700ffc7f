"""The polar / log8 codecs (csrc/smx_quant.hip) and the members of zero_materialize on the GPU.

Codes are held to the float64 definitions of tests/quant_common.py by its rule (exact outside a band of 1e-4 code units
around a rounding boundary, at most one off inside; at most 0.2 % of an input inside the band, asserted from float64 alone),
FOR THE RANGE THE CODE UNDER TEST USED; the range itself to 4 fp32 ulps; decoded values and the transform-based ops to the
project's TOL_ACT / TOL_PARAM, max-normalised (log8_decode: per element, relative).  Every figure is printed before it is
asserted.

Which size reaches which part of a walk (a group is four elements from the first 16-byte address of the wide side on):
  n = 1, 15, 16, 17, 255     no group / three groups and a tail / four groups / a tail of one / 63 groups and a tail
                             (n = 1 is a constant-magnitude input: its magnitude code must be 0, its phase code obeys the rule)
  n = 4099, (3, 1000)        more than one workgroup's worth of groups (1024 per workgroup and round)
  z[1:]                      the wide side 8 bytes off: a head element, planes read / written from byte 1 on
  planes at +1 and +3        four byte accesses per lane instead of one dword
  n = 3 * 4096 + 5 under max_workgroups 1 and 2: every workgroup walks several rounds and workgroup 0 the ragged ends"""
import numpy as np
import pytest
import torch

import quant_common as qc
from conftest import TOL_ACT, TOL_PARAM, load_golden, rel_err

pytestmark = pytest.mark.gpu

SIZES = [(1,), (15,), (16,), (17,), (255,), (4099,), (3, 1000)]
NATIVE_CONFIGS = [(4, 8), (3, 5), (1, 1), (8, 8)]
GUARD = 0xA5


def _fn():
    from tensor_cuda_fft_amd import functional as fn
    return fn


def _show(name, value, bound):
    print(f"{name}: {value:.3g} (bound {bound:.3g})")
    return value


def _check_range(rng, z):
    want = qc.polar_range_def(z)
    tol = 4 * qc.ulp32(max(abs(want[0]), abs(want[1])))
    for end, got, w in zip(("min", "max"), rng, want):
        assert _show(f"range {end} |delta|", abs(got - w), tol) <= tol


def _check_polar_codes(tag, mag_q, phase_q, z, config, rng):
    mb, pb = config
    u, v = qc.polar_uv_def(z, mb, pb, rng)
    share = max(qc.band_share(u, "round"), qc.band_share(v, "round"))
    assert _show(f"{tag} share of elements in the band", share, qc.BAND_SHARE) <= qc.BAND_SHARE
    if z.numel() == 1:          # one magnitude: 1 / (max - min + 1e-9) amplifies its last bit without limit; the code is 0
        assert int(mag_q.max()) == 0
        fm, wm = 0, 0.0
    else:
        assert rng[1] - rng[0] >= 1.0, "the input must span at least one octave of magnitude"
        fm, wm = qc.check_codes(mag_q, u, 2 ** mb - 1, "round")
    fp, wp = qc.check_codes(phase_q, v, 2 ** pb - 1, "round")
    print(f"{tag}: {fm} magnitude and {fp} phase codes differ from float64's, worst distance {max(wm, wp):.3g} (band {qc.BAND})")


def _check_deq(tag, out, mag_q, phase_q, config, rng):
    e = rel_err(out.cpu().numpy(), qc.polar_dequantize_def(mag_q, phase_q, *config, rng))
    assert _show(f"{tag} dequantize", e, TOL_ACT) <= TOL_ACT


# ---- polar ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("config", NATIVE_CONFIGS, ids=lambda c: "%d_%d" % c)
@pytest.mark.parametrize("shape", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_polar_codec(gpu, shape, config):
    fn = _fn()
    z = qc.polar_input(shape)
    zd = z.to(gpu)
    r = fn.polar_range(zd)
    assert r.dtype == torch.float32 and r.shape == (2,) and r.device == zd.device
    rng = tuple(r.tolist())
    _check_range(rng, z)
    mag_q, phase_q = fn.polar_quantize(zd, *config, rng)
    assert mag_q.dtype == phase_q.dtype == torch.uint8 and mag_q.shape == phase_q.shape == z.shape
    _check_polar_codes(f"polar {shape} {config}", mag_q, phase_q, z, config, rng)
    out = fn.polar_dequantize(mag_q, phase_q, *config, rng)
    assert out.dtype == torch.complex64 and out.shape == z.shape
    _check_deq(f"polar {shape} {config}", out, mag_q, phase_q, config, rng)


def _raw_polar(gpu, z, config, rng, z_off, m_off, p_off, mwg=0):
    """quantize and dequantize through the C entries with the wide side z_off ELEMENTS and the planes m_off / p_off BYTES
    into guarded buffers; returns the codes and the decoded tensor after checking that no guard byte changed"""
    from tensor_cuda_fft_amd import _lib
    L, n = _lib.lib(), z.numel()
    s = torch.cuda.current_stream().cuda_stream
    zb = torch.full((n + z_off + 2,), complex(7.0, 7.0), dtype=torch.complex64, device=gpu)
    zb[z_off:z_off + n] = z.reshape(-1).to(gpu)
    assert zb.data_ptr() % 16 == 0
    mb = torch.full((n + m_off + 8,), GUARD, dtype=torch.uint8, device=gpu)
    pb = torch.full((n + p_off + 8,), GUARD, dtype=torch.uint8, device=gpu)
    _lib.check(L.smx_polar_quantize(zb.data_ptr() + 8 * z_off, mb.data_ptr() + m_off, pb.data_ptr() + p_off, n, *config,
                                    rng[0], rng[1], mwg, s))
    for buf, off in ((mb, m_off), (pb, p_off)):
        assert bool((buf[:off] == GUARD).all()) and bool((buf[off + n:] == GUARD).all()), "a plane was written out of bounds"
    ob = torch.full((n + z_off + 2,), complex(7.0, 7.0), dtype=torch.complex64, device=gpu)
    _lib.check(L.smx_polar_dequantize(mb.data_ptr() + m_off, pb.data_ptr() + p_off, ob.data_ptr() + 8 * z_off, n, *config,
                                      rng[0], rng[1], mwg, s))
    assert bool((ob[:z_off] == complex(7.0, 7.0)).all()) and bool((ob[z_off + n:] == complex(7.0, 7.0)).all())
    return mb[m_off:m_off + n].clone(), pb[p_off:p_off + n].clone(), ob[z_off:z_off + n].clone()


@pytest.mark.parametrize("offsets", [(1, 0, 0), (0, 1, 3), (1, 3, 1), (1, 1, 0)], ids=lambda o: "z%d_m%d_p%d" % o)
@pytest.mark.parametrize("n", [2, 17, 4099])
def test_polar_views_and_offset_planes(gpu, n, offsets):
    fn = _fn()
    z = qc.polar_input((4099,))[:n]
    rng = tuple(fn.polar_range(z.to(gpu)).tolist())
    base = fn.polar_quantize(z.to(gpu), 4, 8, rng)
    mq, pq, out = _raw_polar(gpu, z, (4, 8), rng, *offsets)
    assert torch.equal(mq, base[0]) and torch.equal(pq, base[1]), "codes depend on the alignment"
    assert torch.equal(torch.view_as_real(out), torch.view_as_real(fn.polar_dequantize(*base, 4, 8, rng)))
    # the same through functional: views are read in place
    zb = torch.zeros(n + 1, dtype=torch.complex64, device=gpu)
    zb[1:] = z.to(gpu)
    assert zb[1:].data_ptr() % 16 == 8
    assert torch.equal(fn.polar_range(zb[1:]), torch.tensor(rng, device=gpu))
    got = fn.polar_quantize(zb[1:], 4, 8, rng)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    if n > 3:
        assert torch.equal(torch.view_as_real(fn.polar_dequantize(base[0][3:], base[1][1:n - 2], 4, 8, rng)),
                           torch.view_as_real(fn.polar_dequantize(base[0][3:].clone(), base[1][1:n - 2].clone(), 4, 8, rng)))


@pytest.mark.parametrize("mwg", [1, 2])
def test_polar_under_a_workgroup_cap(gpu, mwg):
    fn = _fn()
    n = 3 * 4096 + 5
    z = qc.polar_input((n,))
    zd = z.to(gpu)
    r = fn.polar_range(zd, max_workgroups=mwg)
    assert torch.equal(r, fn.polar_range(zd))
    rng = tuple(r.tolist())
    _check_range(rng, z)
    mag_q, phase_q = fn.polar_quantize(zd, 4, 8, rng, max_workgroups=mwg)
    free = fn.polar_quantize(zd, 4, 8, rng)
    assert torch.equal(mag_q, free[0]) and torch.equal(phase_q, free[1])
    _check_polar_codes(f"polar n={n} mwg={mwg}", mag_q, phase_q, z, (4, 8), rng)
    out = fn.polar_dequantize(mag_q, phase_q, 4, 8, rng, max_workgroups=mwg)
    assert torch.equal(torch.view_as_real(out), torch.view_as_real(fn.polar_dequantize(mag_q, phase_q, 4, 8, rng)))
    _check_deq(f"polar n={n} mwg={mwg}", out, mag_q, phase_q, (4, 8), rng)
    mq, pq, _ = _raw_polar(gpu, z, (4, 8), rng, 1, 3, 1, mwg=mwg)
    assert torch.equal(mq, mag_q.reshape(-1)) and torch.equal(pq, phase_q.reshape(-1))


def test_polar_special_values(gpu):
    fn = _fn()
    z = qc.special_polar()
    zd = z.to(gpu)
    rng = tuple(fn.polar_range(zd).tolist())
    _check_range(rng, z)
    assert abs(rng[0] - np.log2(1e-9)) < 1e-5 and abs(rng[1] - np.log2(1e15)) < 1e-4
    mag_q, phase_q = fn.polar_quantize(zd, 8, 8, rng)
    _check_polar_codes("special values", mag_q, phase_q, z, (8, 8), rng)
    m, p = mag_q.cpu().tolist(), phase_q.cpu().tolist()
    assert m[0] == m[5] == m[6] == 0 and m[7] == 255                # (+0, +0) and |z| = 1e-12 clamp to the bottom code
    assert p[0] in (127, 128) and p[1] in (127, 128) and p[3] == 255 and (p[2], p[4]) == (191, 64)
    zneg = torch.tensor([complex(-1.0, -0.0)], dtype=torch.complex64, device=gpu)
    assert fn.polar_quantize(zneg, 8, 8, rng)[1].item() == 0        # atan2(-0, -1) = -pi
    _check_deq("special values", fn.polar_dequantize(mag_q, phase_q, 8, 8, rng), mag_q, phase_q, (8, 8), rng)


def test_polar_constant_magnitude(gpu):
    fn = _fn()
    zd = qc.constant_magnitude().to(gpu)
    rng = tuple(fn.polar_range(zd).tolist())
    assert rng[0] == rng[1]
    _check_range(rng, qc.constant_magnitude())
    mag_q, _ = fn.polar_quantize(zd, 4, 8, rng)
    assert int(mag_q.max()) == 0


@pytest.mark.parametrize("config", NATIVE_CONFIGS, ids=lambda c: "%d_%d" % c)
def test_polar_dequantize_all_code_pairs(gpu, config):
    fn = _fn()
    mb, pb = config
    mq = torch.arange(2 ** mb, dtype=torch.uint8).repeat_interleave(2 ** pb)
    pq = torch.arange(2 ** pb, dtype=torch.uint8).repeat(2 ** mb)
    rng = (-7.25, 1.5)
    out = fn.polar_dequantize(mq.to(gpu), pq.to(gpu), mb, pb, rng)
    _check_deq(f"all {mq.numel()} code pairs of {config}", out, mq, pq, config, rng)


@pytest.mark.parametrize("config", qc.POLAR_CONFIGS, ids=lambda c: "%d_%d" % c)
@pytest.mark.parametrize("shape", qc.POLAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_polar_round_trip_is_the_format_s_error(gpu, shape, config):
    """PolarQuantizer on the device, (6, 10) on the composition of torch ops; the error is that of the format"""
    import tensor_cuda_fft_amd as pkg
    g = load_golden(qc.polar_name(shape))
    z = qc.polar_input(shape)
    q = pkg.PolarQuantizer(*config)
    zd = z.to(gpu)
    mag_q, phase_q = q.quantize(zd)
    assert isinstance(q.mag_range, tuple) and all(type(v) is float for v in q.mag_range)
    _check_range(q.mag_range, z)
    first = q.mag_range
    q.quantize(zd * 64)
    assert q.mag_range == first
    out = q.dequantize(mag_q, phase_q)
    assert out.is_cuda and out.dtype == torch.complex64
    e = (torch.norm(out.cpu() - z) / torch.norm(z)).item()
    bound = 1.05 * float(g["rt_err.%d_%d" % config])
    assert _show(f"round trip {shape} {config}", e, bound) <= bound


# ---- log8 -----------------------------------------------------------------------------------------------------------------------

def _check_log8_codes(tag, enc, x):
    sign, t = qc.log8_t_def(x)
    share = qc.band_share(t, "trunc")
    assert _show(f"{tag} share of elements in the band", share, qc.BAND_SHARE) <= qc.BAND_SHARE
    e = enc.cpu().numpy().astype(np.int64).reshape(sign.shape)
    assert np.array_equal(e >> 7, sign)
    flips, worst = qc.check_codes(e & 127, t, 127, "trunc")
    print(f"{tag}: {flips} codes differ from float64's, worst distance {worst:.3g} (band {qc.BAND})")


def _check_log8_values(tag, x, codes):
    want = qc.log8_decode_def(codes)
    e = float(np.max(np.abs(x.cpu().numpy().astype(np.float64) / want - 1)))
    assert _show(f"{tag} decode, largest relative error", e, TOL_ACT) <= TOL_ACT


@pytest.mark.parametrize("shape", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_log8_codec(gpu, shape):
    fn = _fn()
    x = qc.log8_input(shape)
    enc = fn.log8_encode(x.to(gpu))
    assert enc.dtype == torch.uint8 and enc.shape == x.shape
    _check_log8_codes(f"log8 {shape}", enc, x)
    dec = fn.log8_decode(enc)
    assert dec.dtype == torch.float32 and dec.shape == x.shape
    _check_log8_values(f"log8 {shape}", dec, enc.cpu())
    z = torch.complex(x, qc.log8_input(shape, qc.SEED + 1))
    re_q, im_q = fn.log8_encode_complex(z.to(gpu))
    assert torch.equal(re_q, enc)
    _check_log8_codes(f"log8 complex {shape}", im_q, z.imag)
    back = fn.log8_decode_complex(re_q, im_q)
    assert back.dtype == torch.complex64 and back.shape == z.shape
    assert torch.equal(back.real, dec) and torch.equal(back.imag, fn.log8_decode(im_q))


def test_log8_all_codes_and_special_values(gpu):
    fn = _fn()
    codes = torch.arange(256, dtype=torch.uint8)
    _check_log8_values("all 256 codes", fn.log8_decode(codes.to(gpu)), codes)
    sp = torch.tensor([0.0, -0.0, 1e-30, 1e30, -1e30, -1e-30], device=gpu)
    assert fn.log8_encode(sp).tolist() == [128, 128, 128, 255, 127, 0]


@pytest.mark.parametrize("mwg", [0, 1, 2])
@pytest.mark.parametrize("x_off", [0, 1, 2, 3])
def test_log8_views_offset_planes_and_caps(gpu, x_off, mwg):
    """fp32 heads of 0..3 elements, the plane 0..3 bytes off, through the C entries into guarded buffers"""
    from tensor_cuda_fft_amd import _lib
    fn = _fn()
    L, n = _lib.lib(), 3 * 4096 + 5
    s = torch.cuda.current_stream().cuda_stream
    x = qc.log8_input((n,))
    base = fn.log8_encode(x.to(gpu))
    _check_log8_codes(f"log8 n={n}", base, x)
    p_off = (x_off + 1) % 4
    xb = torch.zeros(n + x_off + 4, device=gpu)
    xb[x_off:x_off + n] = x.to(gpu)
    eb = torch.full((n + p_off + 8,), GUARD, dtype=torch.uint8, device=gpu)
    _lib.check(L.smx_log8_encode(xb.data_ptr() + 4 * x_off, eb.data_ptr() + p_off, n, mwg, s))
    assert bool((eb[:p_off] == GUARD).all()) and bool((eb[p_off + n:] == GUARD).all())
    assert torch.equal(eb[p_off:p_off + n], base)
    ob = torch.full((n + x_off + 4,), 7.0, device=gpu)
    _lib.check(L.smx_log8_decode(eb.data_ptr() + p_off, ob.data_ptr() + 4 * x_off, n, mwg, s))
    assert bool((ob[:x_off] == 7.0).all()) and bool((ob[x_off + n:] == 7.0).all())
    assert torch.equal(ob[x_off:x_off + n], fn.log8_decode(base))
    # the complex pair: the wide side 8 bytes off when x_off is odd
    z = torch.complex(x, qc.log8_input((n,), qc.SEED + 1))
    want = fn.log8_encode_complex(z.to(gpu))
    zb = torch.zeros(n + 2, dtype=torch.complex64, device=gpu)
    z_off = x_off % 2
    zb[z_off:z_off + n] = z.to(gpu)
    rb = torch.full((n + 12,), GUARD, dtype=torch.uint8, device=gpu)
    ib = torch.full((n + 12,), GUARD, dtype=torch.uint8, device=gpu)
    i_off = 3 - p_off
    _lib.check(L.smx_log8_encode_c64(zb.data_ptr() + 8 * z_off, rb.data_ptr() + p_off, ib.data_ptr() + i_off, n, mwg, s))
    for buf, off, w in ((rb, p_off, want[0]), (ib, i_off, want[1])):
        assert bool((buf[:off] == GUARD).all()) and bool((buf[off + n:] == GUARD).all())
        assert torch.equal(buf[off:off + n], w)
    zo = torch.full((n + 2,), complex(7.0, 7.0), dtype=torch.complex64, device=gpu)
    _lib.check(L.smx_log8_decode_c64(rb.data_ptr() + p_off, ib.data_ptr() + i_off, zo.data_ptr() + 8 * z_off, n, mwg, s))
    assert bool((zo[:z_off] == complex(7.0, 7.0)).all()) and bool((zo[z_off + n:] == complex(7.0, 7.0)).all())
    assert torch.equal(torch.view_as_real(zo[z_off:z_off + n]), torch.view_as_real(fn.log8_decode_complex(*want)))


def test_log8_quantizer_on_the_device(gpu):
    import tensor_cuda_fft_amd as pkg
    g = load_golden("R21_log8")
    z, idx = torch.from_numpy(g["c.z"]).to(gpu), torch.from_numpy(g["c.indices"]).to(gpu)
    re_q, im_q = pkg.LogarithmicQuantizer.compress_sparse_freq(z, idx)
    _check_log8_codes("compress_sparse_freq re", re_q, torch.from_numpy(g["c.z"]).real)
    out = pkg.LogarithmicQuantizer.decompress_sparse_freq(re_q, im_q, idx, (64,))
    assert out.is_cuda and out.dtype == torch.complex64 and out.shape == (64,)
    if torch.equal(re_q.cpu(), torch.from_numpy(g["c.re_q"])) and torch.equal(im_q.cpu(), torch.from_numpy(g["c.im_q"])):
        e = rel_err(out.cpu().numpy(), g["c.out"])
        assert _show("decompress_sparse_freq", e, TOL_ACT) <= TOL_ACT


# ---- reproducibility, capture, refusals -----------------------------------------------------------------------------------------

def test_two_runs_and_a_graph_replay_are_bitwise_equal(gpu):
    fn = _fn()
    z = qc.polar_input((4099,)).to(gpu)
    x = qc.log8_input((4099,)).to(gpu)
    rng = tuple(fn.polar_range(z).tolist())

    def run():
        r = fn.polar_range(z)
        mq, pq = fn.polar_quantize(z, 4, 8, rng)
        d = fn.polar_dequantize(mq, pq, 4, 8, rng)
        e = fn.log8_encode(x)
        re_q, im_q = fn.log8_encode_complex(z)
        return [r, mq, pq, torch.view_as_real(d), e, fn.log8_decode(e), re_q, im_q,
                torch.view_as_real(fn.log8_decode_complex(re_q, im_q))]
    a, b = run(), run()
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            c = run()
    torch.cuda.current_stream().wait_stream(side)
    for t in c:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(a, c))


def test_raw_entries_refuse_bad_arguments(gpu):
    from tensor_cuda_fft_amd import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    n = 40
    z = torch.ones(n, dtype=torch.complex64, device=gpu)
    x = torch.ones(n, device=gpu)
    a = torch.full((n,), 9, dtype=torch.uint8, device=gpu)
    b = torch.full((n,), 9, dtype=torch.uint8, device=gpu)
    out2 = torch.full((2,), 7.0, device=gpu)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=gpu)
    zp, xp, ap, bp = z.data_ptr(), x.data_ptr(), a.data_ptr(), b.data_ptr()
    INV = _lib.SMX_ERR_INVALID
    for bits in ((0, 8), (9, 8), (4, 0), (4, 9), (-1, 4)):
        assert L.smx_polar_quantize(zp, ap, bp, n, *bits, 0.0, 1.0, 0, s) == INV and b"1..8" in L.smx_last_error()
        assert L.smx_polar_dequantize(ap, bp, zp, n, *bits, 0.0, 1.0, 0, s) == INV
    assert L.smx_polar_quantize(None, ap, bp, n, 4, 8, 0.0, 1.0, 0, s) == INV
    assert L.smx_polar_quantize(zp, None, bp, n, 4, 8, 0.0, 1.0, 0, s) == INV
    assert L.smx_polar_quantize(zp, ap, None, n, 4, 8, 0.0, 1.0, 0, s) == INV
    assert L.smx_polar_quantize(zp, ap, bp, -1, 4, 8, 0.0, 1.0, 0, s) == INV
    assert L.smx_polar_quantize(zp, ap, bp, n, 4, 8, 0.0, 1.0, -1, s) == INV
    assert L.smx_polar_quantize(zp + 4, ap, bp, n - 1, 4, 8, 0.0, 1.0, 0, s) == INV and b"aligned" in L.smx_last_error()
    assert L.smx_polar_dequantize(ap, bp, None, n, 4, 8, 0.0, 1.0, 0, s) == INV
    assert L.smx_polar_dequantize(None, bp, zp, n, 4, 8, 0.0, 1.0, 0, s) == INV
    assert L.smx_polar_range(None, n, out2.data_ptr(), ws.data_ptr(), ws.numel(), 0, s) == INV
    assert L.smx_polar_range(zp, n, None, ws.data_ptr(), ws.numel(), 0, s) == INV
    assert L.smx_polar_range(zp, n, out2.data_ptr(), None, 0, 0, s) == INV
    assert L.smx_polar_range(zp, n, out2.data_ptr(), ws.data_ptr(), 8, 0, s) == INV
    assert L.smx_polar_range(zp, n, out2.data_ptr(), ws.data_ptr() + 8, ws.numel() - 8, 0, s) == INV
    assert L.smx_polar_range(zp, -1, out2.data_ptr(), ws.data_ptr(), ws.numel(), 0, s) == INV
    assert L.smx_log8_encode(None, ap, n, 0, s) == INV and L.smx_log8_encode(xp, None, n, 0, s) == INV
    assert L.smx_log8_encode(xp + 2, ap, n - 1, 0, s) == INV
    assert L.smx_log8_decode(None, xp, n, 0, s) == INV and L.smx_log8_decode(ap, None, n, 0, s) == INV
    assert L.smx_log8_decode(ap, xp, n, -1, s) == INV
    assert L.smx_log8_encode_c64(zp, ap, None, n, 0, s) == INV and L.smx_log8_encode_c64(zp, ap, bp, -2, 0, s) == INV
    assert L.smx_log8_decode_c64(ap, None, zp, n, 0, s) == INV and L.smx_log8_decode_c64(ap, bp, zp + 4, n - 1, 0, s) == INV
    # zero-sized: success, nothing enqueued, nothing touched (NULL pointers are fine then)
    assert L.smx_polar_range(None, 0, None, None, 0, 0, s) == 0
    assert L.smx_polar_quantize(None, None, None, 0, 4, 8, 0.0, 1.0, 0, s) == 0
    assert L.smx_polar_dequantize(None, None, None, 0, 4, 8, 0.0, 1.0, 0, s) == 0
    assert L.smx_log8_encode(None, None, 0, 0, s) == 0 and L.smx_log8_decode(None, None, 0, 0, s) == 0
    assert L.smx_log8_encode_c64(None, None, None, 0, 0, s) == 0 and L.smx_log8_decode_c64(None, None, None, 0, 0, s) == 0
    torch.cuda.synchronize()
    assert bool((a == 9).all()) and bool((b == 9).all()) and bool((out2 == 7.0).all())
    assert bool((z == 1).all()) and bool((x == 1).all())


def test_everything_else_runs_the_reference_s_ops_on_the_device(gpu):
    """bit counts above 8, other dtypes and inputs that require grad take the composition (same results as on the CPU up to
    the device's own rounding: the codes obey the same rule)"""
    fn = _fn()
    z = qc.polar_input((3, 1000))
    zd = z.to(gpu)
    rng = tuple(fn.polar_range(zd).tolist())
    mq, pq = fn.polar_quantize(zd.clone().requires_grad_(True), 4, 8, rng)
    _check_polar_codes("composition (requires grad)", mq, pq, z, (4, 8), rng)
    mq, _ = fn.polar_quantize(zd, 6, 10, rng)
    u, _ = qc.polar_uv_def(z, 6, 10, rng)
    qc.check_codes(mq, u, 63, "round")
    z128 = zd.to(torch.complex128)
    r128 = fn.polar_range(z128)
    assert r128.dtype == torch.float64
    _check_range(tuple(r128.tolist()), z)
    x64 = qc.log8_input((255,)).double()
    _check_log8_codes("log8 float64", fn.log8_encode(x64.to(gpu)), x64)


# ---- the transform-based ops ----------------------------------------------------------------------------------------------------

def _grads_def(f, *ts, g):
    leaves = [qc.c128(t).clone().requires_grad_(True) for t in ts]
    y = f(*leaves)
    return y.detach(), torch.autograd.grad(y, leaves, g.double())


def _check_op(gpu, tag, f_gpu, f_def, ts, param_from=1):
    """values and every gradient of f_gpu(*ts on the device) against f_def in complex128 / float64"""
    g = torch.randn(f_def(*[qc.c128(t) for t in ts]).shape, generator=torch.Generator().manual_seed(9))
    y64, grads64 = _grads_def(f_def, *ts, g=g)
    leaves = [t.to(gpu).requires_grad_(True) for t in ts]
    y = f_gpu(*leaves)
    assert y.dtype == torch.float32 and y.shape == y64.shape
    assert _show(f"{tag} y", rel_err(y.detach().cpu().numpy(), y64.numpy()), TOL_ACT) <= TOL_ACT
    grads = torch.autograd.grad(y, leaves, g.to(gpu))
    for i, (got, want) in enumerate(zip(grads, grads64)):
        tol = TOL_ACT if i < param_from else TOL_PARAM
        assert got.dtype == ts[i].dtype
        assert _show(f"{tag} grad {i}", rel_err(got.cpu().numpy(), want.numpy()), tol) <= tol


@pytest.mark.parametrize("dims", [(2, 5, 16, 16), (2, 3, 12, 20), (2, 5, 16, 24)], ids=lambda d: "x".join(map(str, d)))
def test_frequency_linear_values_and_gradients(gpu, dims):
    import tensor_cuda_fft_amd as pkg
    x, w, b = qc.linear_inputs(*dims)
    _check_op(gpu, f"frequency_linear {dims}", pkg.frequency_linear, qc.linear_def, (x, w, b))
    y = pkg.ConvolutionTheoremMatMul.frequency_linear_batched(x.to(gpu), w.to(gpu), b.to(gpu), chunk_size=1)
    assert rel_err(y.cpu().numpy(), qc.linear_def(x, w, b).numpy()) <= TOL_ACT
    assert rel_err(pkg.frequency_linear(x.to(gpu), w.to(gpu)).cpu().numpy(), qc.linear_def(x, w).numpy()) <= TOL_ACT


def test_frequency_linear_with_a_complex_input(gpu):
    import tensor_cuda_fft_amd as pkg
    x, w, b = qc.linear_inputs(2, 3, 16, 16, complex_x=True)
    _check_op(gpu, "frequency_linear complex x", pkg.frequency_linear, qc.linear_def, (x, w, b))


@pytest.mark.parametrize("learn_phase", (True, False))
def test_frequency_linear_layer(gpu, learn_phase):
    import tensor_cuda_fft_amd as pkg
    torch.manual_seed(3)
    layer = pkg.FrequencyLinearLayer(16, 16, sparsity=0.5, learn_phase=learn_phase)
    with torch.no_grad():
        layer.bias.normal_()
    x = torch.randn(2, 5, 16, generator=torch.Generator().manual_seed(4))
    if learn_phase:
        ts = (x, layer.weight_freq.detach().clone(), layer.bias.detach().clone())
        f_def = qc.linear_def
    else:
        ts = (x, layer.weight_magnitude.detach().clone(), layer.bias.detach().clone())
        phase = layer.weight_phase.double()
        f_def = lambda a, m, c: qc.linear_def(a, m * torch.exp(1j * phase), c)            # noqa: E731
    layer = layer.to(gpu)
    names = ["weight_freq" if learn_phase else "weight_magnitude", "bias"]

    def f_gpu(a, m, c):
        with torch.no_grad():
            getattr(layer, names[0]).copy_(m)
            layer.bias.copy_(c)
        y = layer(a)
        f_gpu.params = [getattr(layer, n) for n in names]
        return y
    g = torch.randn(2, 5, 16, generator=torch.Generator().manual_seed(9))
    y64, grads64 = _grads_def(f_def, *ts, g=g)
    xd = x.to(gpu).requires_grad_(True)
    y = f_gpu(xd, ts[1].to(gpu), ts[2].to(gpu))
    assert _show("layer y", rel_err(y.detach().cpu().numpy(), y64.numpy()), TOL_ACT) <= TOL_ACT
    grads = torch.autograd.grad(y, [xd] + f_gpu.params, g.to(gpu))
    for i, (got, want) in enumerate(zip(grads, grads64)):
        tol = TOL_ACT if i == 0 else TOL_PARAM
        assert _show(f"layer grad {i}", rel_err(got.cpu().numpy(), want.numpy()), tol) <= tol


@pytest.mark.parametrize("i", range(len(qc.CONV1D)))
def test_frequency_conv1d_values_and_gradients(gpu, i):
    import tensor_cuda_fft_amd as pkg
    case = qc.CONV1D[i]
    x, w = qc.conv1d_inputs(case)
    _check_op(gpu, f"conv1d {case}", lambda a, c: pkg.frequency_conv1d(a, c, case[6], case[5]),
              lambda a, c: qc.conv_def(a, c, case[6], case[5]), (x, w))


def test_frequency_conv2d_values_and_gradients(gpu):
    import tensor_cuda_fft_amd as pkg
    x, w = qc.conv2d_inputs()
    st, pad = qc.CONV2D[8], qc.CONV2D[7]
    _check_op(gpu, "conv2d", lambda a, c: pkg.ConvolutionTheoremMatMul.frequency_conv2d(a, c, st, pad),
              lambda a, c: qc.conv_def(a, c, st, pad), (x, w))


def test_frequency_conv3d_values_and_gradients(gpu):
    import tensor_cuda_fft_amd as pkg
    x, w = qc.conv3d_inputs()
    _check_op(gpu, "conv3d", pkg.ConvolutionTheoremMatMul.frequency_conv3d, lambda a, c: qc.conv_def(a, c, 1, 0), (x, w))


def test_frequency_linear_forms_no_broadcast_product(gpu):
    """(8, 256, 512 -> 512): the reference's complex (B, N, D_in, D_out) product would be 4.3 GB"""
    import tensor_cuda_fft_amd as pkg
    g = torch.Generator().manual_seed(1)
    x = torch.randn(8, 256, 512, generator=g).to(gpu)
    w = (qc.crandn(g, 512, 512) / 512 ** 0.5).to(gpu)
    b = torch.zeros(512, device=gpu)
    pkg.frequency_linear(x[:1], w, b)                         # tables and workspaces of the shape exist
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    before = torch.cuda.memory_allocated(gpu)
    y = pkg.frequency_linear(x, w, b)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(gpu) - before
    assert y.shape == (8, 256, 512)
    assert _show("peak memory rise, MiB", rise / 2 ** 20, 64) < 64
