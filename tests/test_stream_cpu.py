"""FixedSpectralLM and the overlap-save chunk update without a GPU: the state_dict contract, the CPU forward, the torch
path of tensor_cuda_fft_amd.streaming against the fixtures the REFERENCE produced (tests/golden/make_golden_stream.py:
X01 ring wrap, X02 16-row chunks, X03 a token at a time, X04 the L = 143 segment, X05 under a cutoff), the argument
checks of the module and of the two library entries."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import stream_common as sc
from conftest import ROOT, TOL_ACT, load_golden, rel_err

CASES = ["X01_stream_2x48x32_k8_c4", "X02_stream_1x64x36_k16_c16", "X03_stream_3x40x6_k5_c1",
         "X04_stream_1x256x260_k128_c16", "X05_stream_cutoff20_2x48x32"]
_fix = {}


def fixture(name):
    if name not in _fix:
        _fix[name] = load_golden(name)
    return _fix[name]


def build(z, device=None):
    import tensor_cuda_fft_amd as pkg
    model = pkg.FixedSpectralLM(sc.fixture_config(z)).eval()
    model.load_state_dict(sc.fixture_sd(z), strict=True)
    return model if device is None else model.to(device)


def run_fixture(z, model, device=None, native=True, ids_as_list=False):
    """init + every recorded chunk through the package; returns what the fixture recorded, and the final states."""
    import tensor_cuda_fft_amd as pkg
    ids, new_ids = sc.t(z["ids"], device), sc.t(z["new_ids"], device)
    st = pkg.init_layer_states(model, ids, int(z["chunk"]), cutoff=sc.fixture_cutoff(z), native=native)
    out = {"h_last0": st.h_last.clone(), "h_out": [], "h_last": []}
    for c in range(new_ids.shape[0]):
        trace = []
        arg = new_ids[c, 0].tolist() if ids_as_list else new_ids[c]
        assert pkg.update_backbone_chunk(model, st, arg, trace=trace) is st
        out["h_out"].append(torch.stack(trace))
        out["h_last"].append(st["h_last"].clone())
    L = int(z["kernel_len"]) - 1 + int(z["chunk"])
    out["h_out"], out["h_last"] = torch.stack(out["h_out"]), torch.stack(out["h_last"])
    out["win_tail"] = torch.stack([s.window()[:, -L:] for s in st.layers])
    out["pooled"] = torch.stack([s.pooled() for s in st.layers])
    return out, st


def check_fixture(z, out):
    for k in ("h_last0", "h_out", "h_last", "win_tail"):
        assert rel_err(out[k].cpu().numpy(), z[k]) <= TOL_ACT, k
    assert rel_err(out["pooled"].cpu().numpy(), z["ctx_sum"] / float(z["seq_len"])) <= TOL_ACT


def test_lm_config_has_the_reference_defaults_and_construction_is_silent(capsys):
    import tensor_cuda_fft_amd as pkg
    c = pkg.LMConfig()
    assert (c.vocab_size, c.d_model, c.n_layers, c.seq_len, c.kernel_len, c.jpeg_transition, c.bicameral,
            c.frequency_native) == (256, 512, 6, 1024, 128, 32, False, False)
    m = pkg.FixedSpectralLM(pkg.LMConfig(d_model=8, n_layers=2, seq_len=16, kernel_len=4))
    assert capsys.readouterr().out == ""
    assert m.cfg.d_model == 8 and len(m.blocks) == 2 and all(type(b) is pkg.FixedSpectralBlock for b in m.blocks)
    for flag, cls in (("bicameral", pkg.BicameralBlock), ("frequency_native", pkg.FrequencyNativeBlock)):
        m = pkg.FixedSpectralLM(pkg.LMConfig(d_model=8, n_layers=1, seq_len=16, kernel_len=4, **{flag: True}))
        assert type(m.blocks[0]) is cls
    assert pkg.ChunkLM(m, 4).head.out_features == 4 * 256               # the backbone ChunkLM asks for


@pytest.mark.parametrize("name", CASES)
def test_state_dict_is_the_reference_s_and_the_cpu_forward_matches(name):
    z = fixture(name)
    import tensor_cuda_fft_amd as pkg
    fresh = pkg.FixedSpectralLM(sc.fixture_config(z))
    assert {k: tuple(v.shape) for k, v in fresh.state_dict().items()} == \
        {k: tuple(v.shape) for k, v in sc.fixture_sd(z).items()}
    model = build(z)
    ids, cut = sc.t(z["ids"]), sc.fixture_cutoff(z)
    with torch.no_grad():
        assert rel_err(model.forward_hidden(ids, cutoff=cut).numpy(), z["hidden"]) <= TOL_ACT
        assert rel_err(model(ids, cutoff=cut).numpy(), z["logits"]) <= TOL_ACT


@pytest.mark.parametrize("name", CASES)
def test_torch_path_matches_the_reference_update(name):
    z = fixture(name)
    out, st = run_fixture(z, build(z))
    assert not st.native
    check_fixture(z, out)


def test_a_list_of_ints_is_the_tensor_form():
    z = fixture("X02_stream_1x64x36_k16_c16")
    model = build(z)
    a, _ = run_fixture(z, model)
    b, _ = run_fixture(z, model, ids_as_list=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_argument_errors():
    import tensor_cuda_fft_amd as pkg
    z = fixture("X01_stream_2x48x32_k8_c4")
    model = build(z)
    ids = sc.t(z["ids"])
    with pytest.raises(ValueError, match="longer than the window"):
        pkg.init_layer_states(model, ids, 42)                            # K - 1 + chunk = 49 > T = 48
    st = pkg.init_layer_states(model, ids, 4)
    with pytest.raises(ValueError, match="new_ids must be"):
        pkg.update_backbone_chunk(model, st, torch.zeros(2, 5, dtype=torch.long))
    with pytest.raises(ValueError, match="new_ids must be"):
        pkg.update_backbone_chunk(model, st, [1, 2, 3, 4])               # a list is one batch row, the states hold two
    with pytest.raises(TypeError, match="integer"):
        pkg.update_backbone_chunk(model, st, torch.zeros(2, 4))
    with pytest.raises(KeyError):
        st["caches"]
    twin = pkg.FixedSpectralLM(pkg.LMConfig(d_model=8, n_layers=1, seq_len=16, kernel_len=4, frequency_native=True))
    with pytest.raises(TypeError, match="only FixedSpectralBlock layers stream"):
        pkg.init_layer_states(twin, torch.zeros(1, 16, dtype=torch.long), 4)


@pytest.mark.parametrize("convert", ["half", "bfloat16", "double", "ln_only"])
def test_a_backbone_that_is_not_fp32_is_refused_before_anything_is_enqueued(convert):
    """The streaming state and both launches are fp32; the decision is taken from the parameters' dtypes."""
    import tensor_cuda_fft_amd as pkg
    z = fixture("X01_stream_2x48x32_k8_c4")
    model = build(z)
    if convert == "ln_only":
        model.blocks[1].ln.half()
    else:
        getattr(model, convert)()
    with pytest.raises(TypeError, match="needs an fp32 backbone"):
        pkg.init_layer_states(model, sc.t(z["ids"]), 4)
    with pytest.raises(ValueError, match="built for seq_len = 48"):
        pkg.init_layer_states(build(z), sc.t(z["ids"])[:, :40], 4)


def test_the_launch_wrappers_refuse_what_the_kernels_cannot_read():
    """stream_push / stream_conv are callable on their own: CPU tensors and other dtypes raise TypeError before a
    pointer is taken (no device needed to see it)."""
    from tensor_cuda_fft_amd import streaming as sm
    ln = torch.nn.LayerNorm(8)
    ring, sums, pos = torch.zeros(1, 16, 8), torch.zeros(1, 2, 8), torch.zeros(1, dtype=torch.int32)
    h = torch.zeros(1, 4, 8)
    with pytest.raises(TypeError, match="ring must be a contiguous torch.float32 tensor on a ROCm device"):
        sm.stream_push(h, ln, ring, sums, pos)
    with pytest.raises(TypeError, match="ring must be"):
        sm.stream_conv(h, ring.half(), pos, torch.zeros(10), torch.zeros(1, 8), ln, 4)
    for bad in (h, h.half(), h.double(), [1.0]):
        with pytest.raises(TypeError, match="must be a float32 tensor on a ROCm device"):
            sm._dense_f32(bad, "h")
    with pytest.raises(TypeError, match="pos must be a contiguous torch.int32"):
        sm._state("pos", pos.long(), torch.int32)


def test_stream_taps_are_the_toeplitz_slice_of_the_effective_response():
    import tensor_cuda_fft_amd as pkg
    z = fixture("X05_stream_cutoff20_2x48x32")
    blk = build(z).blocks[0]
    n_fft, K, chunk = 64, 8, 4
    taps = pkg.stream_taps(blk, n_fft, chunk, cutoff=20)
    p = {k: v.double() for k, v in blk.state_dict().items()}
    h_eff = torch.fft.irfft(sc._response(p, n_fft, 4, 20, torch.float64), n=n_fft)
    assert taps.shape == (K + 2 * chunk - 2,)
    want = torch.stack([h_eff[(i - (chunk - 1)) % n_fft] for i in range(K + 2 * chunk - 2)])
    assert rel_err(taps.numpy(), want.numpy()) <= 1e-6
    assert float(want[:chunk - 1].abs().max()) > 1e-3                    # the wrap is there: negative lags are not zero
    with pytest.raises(ValueError, match="do not fit"):
        pkg.stream_taps(blk, 8, 4)


@pytest.mark.parametrize("use_ema", [False, True])
def test_generate_chunked_is_deterministic_without_a_nucleus(use_ema):
    import tensor_cuda_fft_amd as pkg
    z = fixture("X01_stream_2x48x32_k8_c4")
    torch.manual_seed(3)
    model = pkg.ChunkLM(build(z), 4, use_ema=use_ema, ema_chunk_len=16).eval()
    with torch.no_grad():
        model.head.weight.normal_(0.0, 0.3)
    a = pkg.generate_chunked(model, b"Once upon a time", 5, top_p=1e-9)
    b = pkg.generate_chunked(model, b"Once upon a time", 5, top_p=1e-9, generator=torch.Generator().manual_seed(9))
    assert a == b and isinstance(a, bytes) and len(a) == 48 + 5 * 4
    assert a[:48] == b" " * 32 + b"Once upon a time"
    # the argmax of the penalised logits, chunk by chunk, from the states the module's own pieces give
    st = pkg.init_layer_states(model.backbone, torch.tensor([list(a[:48])]), 4)
    with torch.no_grad():
        last = st.h_last
        if use_ema:
            state = model.ema.scan_tokens(torch.tensor([list(a[:48])]), 16)
            last = last + model.ema_proj(torch.view_as_real(state).reshape(1, -1))
        logits = model.head(last).view(4, 256)
    seen = torch.zeros(256, dtype=torch.bool)
    seen[torch.tensor(list(a[:48]))] = True
    assert list(a[48:52]) == torch.where(seen, logits / 1.15, logits).argmax(dim=1).tolist()
    assert len(pkg.generate_chunked(model, b"x" * 100, 1, top_p=1e-9)) == 48 + 4      # a long prompt keeps its tail


# ---- the library entries, through the pattern of tests/test_abi.py -------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from tensor_cuda_fft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "tensor-cuda-fft-_amd", "csrc", "build.sh")], check=True,
                       capture_output=True)
    return _lib


def test_stream_supported_truth_table(L):
    lib = L.lib()
    sup = lambda T, K, C, chunk: lib.smx_stream_supported(T, K, C, chunk)
    assert sup(1024, 128, 512, 16) == 1 and sup(48, 8, 32, 4) == 1 and sup(40, 5, 6, 1) == 1
    assert [sup(4096, 128, c, 16) for c in (1, 1022, 1023, 1025, 1026, 4096, 4100, 0)] == [1, 1, 1, 0, 0, 1, 0, 0]
    assert [sup(1024, 128, 512, c) for c in (0, 1, 64, 65)] == [0, 1, 1, 0]
    assert [sup(8192, k, 512, 16) for k in (0, 1, 4096, 4097)] == [0, 1, 1, 0]
    assert sup(143, 128, 512, 16) == 1 and sup(142, 128, 512, 16) == 0             # K - 1 + chunk <= T
    assert sup(4, 1, 8, 4) == 1 and sup(3, 1, 8, 4) == 0


def test_stream_entries_validate_without_touching_the_gpu(L):
    lib = L.lib()
    err = lambda: lib.smx_last_error().decode()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p += (-p) % 16                                                                  # a 16-byte aligned address inside buf
    push = lambda h=p, ring=p, sm=p, pos=p, pooled=p, Bt=1, T=48, C=32, chunk=4: \
        lib.smx_stream_push(h, p, p, 1e-5, ring, sm, pos, pooled, Bt, T, C, chunk, None)
    conv = lambda h=p, ring=p, pos=p, taps=p, scale=p, out=p, ff=None, Bt=1, T=48, K=8, C=32, chunk=4: \
        lib.smx_stream_conv(h, ring, pos, taps, scale, p, p, 1e-5, out, ff, Bt, T, K, C, chunk, None)
    for kw in ({"h": None}, {"ring": None}, {"sm": None}, {"pos": None}, {"pooled": None}):
        assert push(**kw) == -1 and "non-NULL" in err()
    for kw in ({"h": None}, {"ring": None}, {"pos": None}, {"taps": None}, {"scale": None}, {"out": None}):
        assert conv(**kw) == -1 and "non-NULL" in err()
    for kw in ({"h": p + 4}, {"ring": p + 8}):
        assert push(**kw) == -1 and "16-byte aligned" in err()
        assert conv(**kw) == -1 and "16-byte aligned" in err()
    assert push(pos=p + 2) == -1 and "4-byte aligned" in err()
    for kw in ({"T": 3}, {"C": 1025}, {"chunk": 65}, {"chunk": 0}, {"Bt": 0}):
        want = "Bt must be" if "Bt" in kw else "unsupported shape"
        assert push(**kw) == -1 and want in err()
        assert conv(**kw) == -1 and want in err()
    assert conv(K=46) == -1 and "unsupported shape" in err()                        # K - 1 + chunk = 49 > T
    assert conv(K=4097, T=8192) == -1 and "unsupported shape" in err()
    hdr = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "generate_chunked_overlap_save.py:101-172" in hdr
