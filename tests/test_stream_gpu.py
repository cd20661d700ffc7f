"""The overlap-save chunk update on the GPU: smx_stream_push / smx_stream_conv through tensor_cuda_fft_amd.streaming
against the fixtures the REFERENCE produced (X01-X05, tests/golden/make_golden_stream.py), the trainer's own shape
against the fp64 restatement of tests/stream_common.py, and the properties the kernels promise: batch rows do not
interact, runs are bitwise reproducible, the compensated window sum does not drift, a captured graph follows the ring."""
import pytest
import torch

import stream_common as sc
from conftest import TOL_ACT, rel_err
from test_stream_cpu import CASES, build, check_fixture, fixture, run_fixture

pytestmark = pytest.mark.gpu


def seeded_model(dev, T, K, C, layers, seed=11, trans=32):
    import tensor_cuda_fft_amd as pkg
    model = pkg.FixedSpectralLM(sc.lm_config(T, K, C, layers, trans)).eval()
    sc.randomize(model, torch.Generator().manual_seed(seed))
    return model.to(dev)


def state_tensors(st):
    out = [st.h_last]
    for s in st.layers:
        out += [s.ring, s.sum, s.pos]
    return out


def same_states(a, b):
    return all(torch.equal(x, y) for x, y in zip(state_tensors(a), state_tensors(b)))


@pytest.mark.parametrize("name", CASES)
def test_native_path_matches_the_reference_update(gpu, name):
    z = fixture(name)
    out, st = run_fixture(z, build(z, gpu), gpu)
    assert st.native
    check_fixture(z, out)
    T, L = int(z["seq_len"]), int(z["kernel_len"]) - 1 + int(z["chunk"])
    for li, s in enumerate(st.layers):                  # ring, sum and pos themselves, through window() / pooled()
        assert s.ring.shape[1] == T and s.sum.shape[1] == 2 and s.pos.dtype == torch.int32
        steps = z["new_ids"].shape[0] * int(z["chunk"])
        assert s.pos.tolist() == [steps % T] * s.ring.shape[0]
        w = s.window()
        assert rel_err(w[:, -L:].cpu().numpy(), z["win_tail"][li]) <= TOL_ACT
        assert rel_err(s.pooled().cpu().numpy(), w.double().mean(dim=1).cpu().numpy()) <= TOL_ACT


def test_torch_path_on_the_gpu_agrees_with_native(gpu):
    z = fixture("X01_stream_2x48x32_k8_c4")
    model = build(z, gpu)
    a, sa = run_fixture(z, model, gpu)
    b, sb = run_fixture(z, model, gpu, native=False)
    assert sa.native and not sb.native
    check_fixture(z, b)
    for k in a:
        assert rel_err(b[k].cpu().numpy(), a[k].cpu().numpy()) <= TOL_ACT, k


def test_the_trainer_s_shape_against_the_fp64_restatement(gpu):
    """Bt = 1, T = 1024, K = 128, C = 512, chunk = 16 (n_fft = 2048), one layer, two chunks: no fixture, the
    reference's op sequence restated in fp64 (tests/stream_common.py) is evaluated here."""
    import tensor_cuda_fft_amd as pkg
    T, K, C, chunk = 1024, 128, 512, 16
    model = seeded_model(gpu, T, K, C, 1)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 256, (1, T), generator=gen)
    new = torch.randint(0, 256, (2, 1, chunk), generator=gen)
    ref = sc.init_ref(sd, ids, 1, 32)
    st = pkg.init_layer_states(model, ids.to(gpu), chunk)
    assert st.native
    assert rel_err(st.h_last.cpu().numpy(), ref["h_last"].numpy()) <= TOL_ACT
    for c in range(2):
        ref, outs = sc.update_ref(sd, ref, new[c], 1, T, 32)
        trace = []
        pkg.update_backbone_chunk(model, st, new[c].to(gpu), trace=trace)
        assert rel_err(trace[0].cpu().numpy(), outs[0].numpy()) <= TOL_ACT
        assert rel_err(st.h_last.cpu().numpy(), ref["h_last"].numpy()) <= TOL_ACT
    assert rel_err(st.layers[0].window().cpu().numpy(), ref["layers"][0]["ctx_ln"].numpy()) <= TOL_ACT
    assert rel_err(st.layers[0].pooled().cpu().numpy(), (ref["layers"][0]["ctx_sum"] / T).numpy()) <= TOL_ACT


def test_batch_rows_do_not_interact_and_runs_are_bitwise_reproducible(gpu):
    import tensor_cuda_fft_amd as pkg
    T, K, C, chunk = 40, 5, 36, 3
    model = seeded_model(gpu, T, K, C, 2)
    gen = torch.Generator().manual_seed(2)
    ids = torch.randint(0, 256, (3, T), generator=gen).to(gpu)
    new = torch.randint(0, 256, (15, 3, chunk), generator=gen).to(gpu)       # 45 rows: past the end of the ring
    st = pkg.init_layer_states(model, ids, chunk)
    rows = [pkg.init_layer_states(model, ids[b:b + 1], chunk) for b in range(3)]
    twin = st.clone()
    for c in range(new.shape[0]):
        pkg.update_backbone_chunk(model, st, new[c])
        pkg.update_backbone_chunk(model, twin, new[c])
        for b in range(3):
            pkg.update_backbone_chunk(model, rows[b], new[c, b:b + 1])
    assert st.native and same_states(st, twin)
    for b in range(3):
        for x, y in zip(state_tensors(st), state_tensors(rows[b])):
            assert torch.equal(x[b:b + 1], y)


# (Bt, chunk, C) -> the instance k_stream_conv<VEC, CH, R> the launcher takes.  VEC, CH: Vec<4> rows for C % 4 == 0 with
# CH = 1, 2, 4, 8, 16 register chunks for C up to 256, 512, 1024, 2048, 4096; the scalar variant otherwise with CH = 1, 4, 16
# for C up to 64, 256, 1023.  R: the largest of 4, 2, 1 with R VEC CH <= 64 accumulator registers AND
# Bt ceil(chunk / R) >= 256 workgroups.
ROW_GROUP_CASES = [(3, 5, 260),       # R = 1: 15 workgroups
                   (64, 16, 36),      # R = 4: 64 x 4 = 256; Vec<4>, one register chunk
                   (128, 5, 260),     # R = 4: 128 x 2 = 256, last group holds ONE row; Vec<4>, two register chunks
                   (100, 5, 36),      # R = 2: 100 x 2 < 256 <= 100 x 3, last group holds one row; Vec<4>
                   (100, 5, 70),      # R = 2, the scalar variant (C % 4 != 0), four register chunks
                   (128, 5, 6),       # R = 4, the scalar variant, C < 64
                   (128, 5, 1024),    # Vec<4> CH 4 R 4: exactly 4 x 4 x 4 = 64 accumulator registers, 128 x 2 = 256
                   (100, 5, 772),     # Vec<4> CH 4 R 2: 100 x 2 < 256 <= 100 x 3; the last vector chunk part-filled
                   (2, 5, 1020),      # Vec<4> CH 4 R 1: 10 workgroups
                   (128, 5, 2048),    # Vec<4> CH 8 R 2: the workgroup count would take 4 (256), 4 x 4 x 8 = 128 registers do not
                   (3, 5, 1540),      # Vec<4> CH 8 R 1: 15 workgroups; ragged last register chunk
                   (128, 5, 2052),    # Vec<4> CH 16 R 1: R forced by the registers (2 x 4 x 16 = 128); ragged
                   (2, 3, 4096),      # Vec<4> CH 16 R 1: the widest row
                   (128, 5, 1023),    # scalar CH 16 R 4: 4 x 1 x 16 = 64 registers, 128 x 2 = 256
                   (100, 5, 258),     # scalar CH 16 R 2: 100 x 2 < 256 <= 100 x 3
                   (3, 5, 1022),      # scalar CH 16 R 1: 15 workgroups
                   (128, 5, 70)]      # scalar CH 4 R 4: 128 x 2 = 256


@torch.no_grad()
def check_the_two_launches(gpu, Bt, chunk, C, T, K):
    from tensor_cuda_fft_amd import streaming as sm
    L = K - 1 + chunk
    gen = torch.Generator().manual_seed(8)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(gpu)
    ln, ffn_ln = torch.nn.LayerNorm(C).to(gpu), torch.nn.LayerNorm(C).to(gpu)
    for q in (ln.weight, ln.bias, ffn_ln.weight, ffn_ln.bias):
        q.copy_(rnd(C))
    ring, hi, h, scale, taps = rnd(Bt, T, C), rnd(Bt, C), rnd(Bt, chunk, C), rnd(Bt, C), rnd(K + 2 * chunk - 2)
    sums = torch.stack((hi, 1e-7 * rnd(Bt, C)), dim=1).contiguous()
    pos = torch.randint(0, T, (Bt,), generator=gen).to(torch.int32)
    pos[:3] = torch.tensor([0, T - 3, T - 1], dtype=torch.int32)[:Bt]        # rows 1 and 2 wrap inside the chunk
    pos = pos.to(gpu)

    def run(sl):
        r, s, p = ring[sl].clone(), sums[sl].clone(), pos[sl].clone()
        pooled = sm.stream_push(h[sl], ln, r, s, p)
        return (r, s, p, pooled) + sm.stream_conv(h[sl], r, p, taps, scale[sl], ffn_ln, K)

    whole = run(slice(0, Bt))
    assert torch.equal(whole[2], (pos + chunk) % T)
    for b in sorted({0, 1, min(2, Bt - 1), Bt // 2, Bt - 1}):
        for x, y in zip(whole, run(slice(b, b + 1))):
            assert torch.equal(x[b:b + 1], y), b
    # and against the plain statement of the step in fp64
    chrono = lambda r, p: r.gather(1, ((p.long().unsqueeze(1) + torch.arange(T, device=gpu)) % T)
                                   .unsqueeze(-1).expand(-1, -1, C))
    new = torch.nn.functional.layer_norm(h.double(), (C,), ln.weight.double(), ln.bias.double(), ln.eps)
    w = torch.cat([chrono(ring, pos).double()[:, chunk:], new], dim=1)
    e = {"ring": rel_err(chrono(whole[0], whole[2]).cpu().numpy(), w.cpu().numpy())}
    tot = sums.double().sum(dim=1) + (new - chrono(ring, pos).double()[:, :chunk]).sum(dim=1)
    e["pooled"] = rel_err(whole[3].cpu().numpy(), (tot / T).cpu().numpy())
    seg = w[:, T - L:]
    if L <= 64:
        y = torch.stack([sum(taps[n + L - 1 - j].double() * seg[:, j] for j in range(L)) for n in range(chunk)], dim=1)
    else:                                                # the same sum as one Toeplitz gather and a matmul
        lag = torch.arange(chunk, device=gpu).unsqueeze(1) + (L - 1 - torch.arange(L, device=gpu)).unsqueeze(0)
        y = torch.matmul(taps.double()[lag], seg)        # (chunk, L) @ (Bt, L, C)
    h_out = h.double() + scale.double().unsqueeze(1) * y
    e["h_out"] = rel_err(whole[4].cpu().numpy(), h_out.cpu().numpy())
    ff = torch.nn.functional.layer_norm(h_out, (C,), ffn_ln.weight.double(), ffn_ln.bias.double(), ffn_ln.eps)
    e["ff_in"] = rel_err(whole[5].cpu().numpy(), ff.cpu().numpy())
    print(f"(Bt, chunk, C, T, K) = ({Bt}, {chunk}, {C}, {T}, {K}): max-normalised distances to fp64 "
          + ", ".join(f"{k} {v:.3e}" for k, v in e.items()) + f"; bound {TOL_ACT:.0e}")
    assert max(e.values()) <= TOL_ACT, e


@pytest.mark.parametrize("Bt,chunk,C", ROW_GROUP_CASES)
def test_the_two_launches_alone_keep_batch_rows_apart(gpu, Bt, chunk, C):
    """The library entries by themselves, on given inputs (no GEMM between them), at every (VEC, CH, R) instance of
    smx_stream_conv: a row of a Bt-row launch is bit for bit that row launched alone (Bt = 1 always runs R = 1, so the
    sums do not depend on R), each at its own ring position, and all rows agree with the plain fp64 statement."""
    check_the_two_launches(gpu, Bt, chunk, C, T=40, K=7)


@pytest.mark.parametrize("Bt", [2, 16])
def test_the_two_launches_at_the_bounds_of_the_tap_table(gpu, Bt):
    """K = 4096 and chunk = 64, the sizes the LDS tap table is made for (4222 taps), over L = 4159 of the T = 4160 ring
    rows, C = 8 (Vec<4>, one register chunk): Bt = 2 runs R = 1 (128 workgroups), Bt = 16 runs R = 4 (16 x 16 = 256)."""
    check_the_two_launches(gpu, Bt, 64, 8, T=4160, K=4096)


@torch.no_grad()
def test_a_half_backbone_is_refused_on_the_gpu_too(gpu):
    import tensor_cuda_fft_amd as pkg
    z = fixture("X01_stream_2x48x32_k8_c4")
    model = build(z, gpu)
    st = pkg.init_layer_states(model, sc.t(z["ids"], gpu), 4)
    before = [x.clone() for x in state_tensors(st)]
    model.half()                                                            # converted behind the states' back
    with pytest.raises(TypeError, match="float32"):
        pkg.update_backbone_chunk(model, st, sc.t(z["new_ids"], gpu)[0])
    assert all(torch.equal(x, y) for x, y in zip(before, state_tensors(st)))          # nothing was written
    with pytest.raises(TypeError, match="needs an fp32 backbone"):
        pkg.init_layer_states(model, sc.t(z["ids"], gpu), 4)


def test_the_compensated_sum_does_not_drift(gpu):
    import tensor_cuda_fft_amd as pkg
    T, K, C, chunk = 48, 8, 32, 4
    model = seeded_model(gpu, T, K, C, 1)
    gen = torch.Generator().manual_seed(4)
    st = pkg.init_layer_states(model, torch.randint(0, 256, (2, T), generator=gen).to(gpu), chunk)
    new = torch.randint(0, 256, (300, 2, chunk), generator=gen).to(gpu)
    for c in range(300):
        pkg.update_backbone_chunk(model, st, new[c])
    s = st.layers[0]
    assert rel_err(s.pooled().cpu().numpy(), s.window().double().mean(dim=1).cpu().numpy()) <= TOL_ACT


def test_a_captured_update_follows_the_ring(gpu):
    """One update captured with a static ids tensor, replayed for three different chunks across the end of the ring
    (pos 40 -> 4 on T = 48): bit for bit the eager run on a cloned state.  The chain is linear: no parallel branches."""
    import tensor_cuda_fft_amd as pkg
    T, K, C, chunk = 48, 8, 32, 4
    model = seeded_model(gpu, T, K, C, 2)
    gen = torch.Generator().manual_seed(6)
    st = pkg.init_layer_states(model, torch.randint(0, 256, (2, T), generator=gen).to(gpu), chunk)
    new = torch.randint(0, 256, (13, 2, chunk), generator=gen).to(gpu)
    for c in range(10):                                                     # warm: pos = 40
        pkg.update_backbone_chunk(model, st, new[c])
    eager = st.clone()
    static_ids = new[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pkg.update_backbone_chunk(model, st, static_ids)
    assert same_states(st, eager)                                           # capturing runs nothing
    for c in range(10, 13):
        static_ids.copy_(new[c])
        graph.replay()
        pkg.update_backbone_chunk(model, eager, new[c])
        torch.cuda.synchronize()
        assert same_states(st, eager), c
    assert st.layers[0].pos.tolist() == [4, 4]


def test_generate_chunked_on_the_gpu_with_and_without_a_graph(gpu):
    import tensor_cuda_fft_amd as pkg
    z = fixture("X01_stream_2x48x32_k8_c4")
    torch.manual_seed(3)
    model = pkg.ChunkLM(build(z), 4, use_ema=True, ema_chunk_len=16).eval()
    with torch.no_grad():
        model.head.weight.normal_(0.0, 0.3)
    model = model.to(gpu)
    a = pkg.generate_chunked(model, b"Once upon a time", 6, top_p=1e-9)
    b = pkg.generate_chunked(model, b"Once upon a time", 6, top_p=1e-9, use_graph=True)
    assert a == b and len(a) == 48 + 6 * 4 and a[:48] == b" " * 32 + b"Once upon a time"
