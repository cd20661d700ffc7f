"""The byte sampler without a GPU: the torch fallback of functional.sample_bytes against the reference's recorded
distributions (tests/golden/Y01_sample_rows.npz) and the fp64 restatement of the definition (tests/sample_common.py), the
argument checks of the Python entry and of the C ABI entry, fixed_spectral.generate against a loop over the restatement,
and generate_chunked(sampler="native") against the torch sampler where both are greedy."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import sample_common as sc
from tensor_cuda_fft_amd.functional import sample_bytes
from test_stream_cpu import build, fixture

R = 512


def run(logits, recent, u, device="cpu", **kw):
    ids, p = sample_bytes(torch.from_numpy(logits).to(device), torch.from_numpy(np.asarray(recent)).to(device),
                          torch.from_numpy(u).to(device), return_probs=True, **kw)
    return ids.cpu().numpy(), p.cpu().numpy()


def check_rows(got_ids, got_p, logits, recent, u, kw, tol=1e-6, what=""):
    """The rules of every comparison: the part left out is bounded; on comparable rows the support is exactly the
    restatement's, the probabilities within tol of it and the ids equal; on ALL rows the id has p > 0 and is not banned."""
    ids, p64, ok = sc.restate(logits, recent, u, **kw)
    print(f"{what}: {sc.share(ok):.3%} of {len(ok)} rows left out, max |p - p64| = {np.abs(got_p[ok] - p64[ok]).max():.2e}")
    assert sc.share(ok) <= sc.MAX_SKIP
    assert np.array_equal(got_p[ok] > 0, p64[ok] > 0)
    assert np.abs(got_p[ok] - p64[ok]).max() <= tol
    assert np.array_equal(got_ids[ok], ids[ok])
    assert (got_p[np.arange(len(got_ids)), got_ids] > 0).all()
    assert not sc.banned(**kw)[got_ids].any()


def test_the_restatement_leaves_out_few_rows():
    """The shares the margin rule costs at the inputs the tests use (3 randn, temperature 0.8)."""
    logits, u = sc.make_rows(R, 21)
    for top_p in (0.9, 0.5):
        ok = sc.restate(logits, sc.make_window(256, 31), u, temperature=0.8, top_p=top_p)[2]
        print(f"top_p {top_p}: {sc.share(ok):.3%} left out")
        assert sc.share(ok) <= 0.05


@pytest.mark.parametrize("name", sorted(sc.SETTINGS))
def test_fallback_equals_the_restatement(name):
    logits, u = sc.make_rows(R, 21)
    recent = sc.make_window(256, 31, run=6 if "max_run" in sc.SETTINGS[name] else 0)
    ids, p = run(logits, recent, u, **sc.SETTINGS[name])
    check_rows(ids, p, logits, recent, u, sc.SETTINGS[name], what=name)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4096])
@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_fallback_windows(n, dtype):
    logits, u = sc.make_rows(64, 22)
    recent = sc.make_window(n, 32 + n, run=6 if n >= 6 else 0).astype(dtype)
    ids, p = run(logits, recent, u, **sc.SETTINGS["all"])
    check_rows(ids, p, logits, recent, u, sc.SETTINGS["all"], what=f"n_recent {n}")


def test_fallback_equals_the_reference_rows():
    z = load_golden("Y01_sample_rows")
    need = {"defaults", "presence_frequency", "topk5_narrow_nucleus", "topk5_wide_nucleus", "run_of_6", "n_recent_0",
            "n_recent_1", "n_recent_300", "top_p_1"}
    assert need <= set(z["cases"].tolist())
    for c in z["cases"].tolist():
        kw = json.loads(str(z[c + ".settings"]))
        ids, p = run(z[c + ".logits"], z[c + ".recent"], z[c + ".u"], **kw)
        ref = z[c + ".probs"]
        assert ref.dtype == np.float32 and len(ref) > 0
        assert np.array_equal(p > 0, ref > 0), c                          # every stored row is comparable
        assert np.abs(p - ref).max() <= 1e-5, c
        check_rows(ids, p, z[c + ".logits"], z[c + ".recent"], z[c + ".u"], kw, what=c)


def test_other_dtypes_and_shapes_run_the_same_definition():
    logits, u = sc.make_rows(12, 23)
    recent = sc.make_window(100, 33)
    kw = sc.SETTINGS["all"]
    ids, p = run(logits, recent, u, **kw)
    l3 = torch.from_numpy(logits).view(3, 4, 256)
    i3, p3 = sample_bytes(l3, torch.from_numpy(recent), torch.from_numpy(u).view(3, 4), return_probs=True, **kw)
    assert i3.shape == (3, 4) and p3.shape == (3, 4, 256) and i3.dtype == torch.int64
    assert np.array_equal(i3.numpy().ravel(), ids) and np.array_equal(p3.numpy().reshape(12, 256), p)
    only = sample_bytes(l3, torch.from_numpy(recent), torch.from_numpy(u).view(3, 4), **kw)
    assert torch.equal(only, i3)
    hb = torch.from_numpy(logits).bfloat16()                              # 2-byte logits: the rows as floats
    ib, pb = sample_bytes(hb, torch.from_numpy(recent), torch.from_numpy(u), return_probs=True, **kw)
    i2, p2 = run(hb.float().numpy(), recent, u, **kw)
    assert np.array_equal(ib.numpy(), i2) and np.array_equal(pb.numpy(), p2)
    # u=None draws from the generator: the same seed, the same bytes; no window at all is allowed
    g = lambda: torch.Generator().manual_seed(5)
    a = sample_bytes(l3, None, generator=g(), temperature=0.8)
    assert torch.equal(a, sample_bytes(l3, None, generator=g(), temperature=0.8)) and a.shape == (3, 4)
    assert sample_bytes(torch.zeros(0, 256), None).shape == (0,)


def test_rounding_never_draws_a_byte_of_probability_zero():
    """u above the last running sum takes the last byte with p > 0; NaN logits give an id in range."""
    logits = np.full((2, 256), -np.inf, np.float32)
    logits[:, 65:68] = 0.0
    ids, p = run(logits, np.zeros(0, np.int64), np.array([0.99999994, 0.0], np.float32))
    assert ids.tolist() == [67, 65] and (p[:, 68:] == 0).all()
    ids, _ = run(logits, np.zeros(0, np.int64), np.array([np.nan, 1.5], np.float32))
    assert ids.tolist() == [67, 67]
    logits[0, 3] = np.nan
    ids, _ = run(logits, np.zeros(0, np.int64), np.array([0.5, 0.5], np.float32), top_p=0.9, top_k=3)
    assert 0 <= ids[0] <= 255 and ids[1] == 66


def test_equal_logits_are_ordered_by_index():
    logits = np.zeros((1, 256), np.float32)                               # all equal: the nucleus keeps bytes 0, 1, 2
    ids, p = run(logits, np.zeros(0, np.int64), np.array([0.5], np.float32), top_p=3.5 / 256)
    assert np.flatnonzero(p[0]).tolist() == [0, 1, 2] and ids[0] == 1


def test_validation_errors():
    l, r, u = torch.zeros(2, 256), torch.zeros(4, dtype=torch.int64), torch.zeros(2)
    with pytest.raises(ValueError, match="256"):
        sample_bytes(torch.zeros(2, 255), r, u)
    with pytest.raises(TypeError, match="floating-point"):
        sample_bytes(torch.zeros(2, 256, dtype=torch.int64), r, u)
    for t in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            sample_bytes(l, r, u, temperature=t)
    with pytest.raises(ValueError, match="repetition_penalty"):
        sample_bytes(l, r, u, repetition_penalty=0.0)
    with pytest.raises(ValueError, match="top_k"):
        sample_bytes(l, r, u, top_k=-1)
    with pytest.raises(ValueError, match="max_run_length"):
        sample_bytes(l, r, u, max_run_length=-1)
    with pytest.raises(ValueError, match="NaN"):
        sample_bytes(l, r, u, top_p=float("nan"))
    with pytest.raises(TypeError, match="recent"):
        sample_bytes(l, r.to(torch.int32), u)
    with pytest.raises(TypeError, match="recent"):
        sample_bytes(l, r.view(2, 2), u)
    with pytest.raises(ValueError, match="65536"):
        sample_bytes(l, torch.zeros(65537, dtype=torch.uint8), u)
    with pytest.raises(ValueError, match="shape"):
        sample_bytes(l, r, torch.zeros(3))


@pytest.fixture(scope="module")
def L():
    from tensor_cuda_fft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "tensor-cuda-fft-_amd", "csrc", "build.sh")], check=True,
                       capture_output=True)
    return _lib


def test_the_entry_refuses_bad_arguments_before_any_launch(L):
    """Every refusal comes before the first HIP call: these run without a GPU."""
    lib = L.lib()
    err = lambda: lib.smx_last_error().decode()
    assert [lib.smx_sample_supported(v) for v in (256, 255, 257, 0, 50257)] == [1, 0, 0, 0, 0]
    buf = (ctypes.c_double * 1024)()
    p = ctypes.addressof(buf)

    def call(logits=p, stride=256, recent=p, tb=8, n=4, temp=0.8, top_p=0.9, top_k=0, rep=1.25, pres=0.0, freq=0.0,
             u=p, ids=p, probs=None, R=1, V=256):
        return lib.smx_sample_bytes(logits, stride, recent, tb, n, temp, top_p, top_k, rep, pres, freq, 1, 1, 6, u, ids,
                                    probs, R, V, None)

    assert call(V=255) == -2 and "256" in err()                           # SMX_ERR_UNSUPPORTED
    assert call(temp=0.0) == -1 and "temperature" in err()                # SMX_ERR_INVALID from here on
    assert call(temp=-1.0) == -1 and call(temp=float("nan")) == -1
    assert call(logits=None) == -1 and "non-NULL" in err()
    assert call(u=None) == -1 and call(ids=None) == -1
    assert call(recent=None) == -1 and "recent" in err()
    assert call(tb=4) == -1 and "token_bytes" in err()
    assert call(stride=255) == -1 and "row_stride" in err()
    assert call(n=-1) == -1 and call(n=65537) == -1 and "n_recent" in err()
    assert call(R=0) == -1 and call(R=1 << 31) == -1
    assert call(rep=0.0) == -1 and "repetition_penalty" in err()
    assert call(top_p=float("nan")) == -1 and call(top_k=-1) == -1 and call(pres=float("inf")) == -1
    assert call(recent=p + 4) == -1 and call(ids=p + 4) == -1 and call(u=p + 2) == -1 and "aligned" in err()


# ---- fixed_spectral.generate and generate_chunked(sampler="native") -------------------------------------------------------
def tiny_lm():
    import tensor_cuda_fft_amd as pkg
    torch.manual_seed(7)
    model = pkg.FixedSpectralLM(pkg.LMConfig(d_model=32, n_layers=2, seq_len=64, kernel_len=8, jpeg_transition=4)).eval()
    with torch.no_grad():
        model.embed.weight.normal_(0.0, 1.5)                              # logits with some spread
    return model


def test_generate_equals_a_loop_over_the_restatement():
    import tensor_cuda_fft_amd as pkg
    model = tiny_lm()
    cfg = pkg.SampleConfig(seq_len=64, max_new=12)
    assert (cfg.temperature, cfg.top_p, cfg.top_k, cfg.repetition_penalty, cfg.repetition_window, cfg.max_run_length,
            cfg.presence_penalty, cfg.frequency_penalty, cfg.ban_cr, cfg.ascii_only, cfg.max_new) == \
        (0.8, 0.9, 0, 1.25, 256, 6, 0.0, 0.0, True, True, 12)
    assert pkg.SampleConfig().max_new == 400 and pkg.SampleConfig().seq_len == 1024
    prompt = "Once upon a time there was a spectral model that read " + "e" * 6
    text = pkg.generate(model, prompt, cfg, generator=torch.Generator().manual_seed(11))
    assert isinstance(text, str) and text.startswith(prompt) and len(text.encode()) == len(prompt) + 12
    # the same uniforms, drawn the same way, through the restatement
    gen = torch.Generator().manual_seed(11)
    ctx = list(prompt.encode())
    kw = dict(temperature=cfg.temperature, top_p=cfg.top_p, top_k=cfg.top_k, repetition_penalty=cfg.repetition_penalty,
              presence_penalty=cfg.presence_penalty, frequency_penalty=cfg.frequency_penalty, ascii_only=cfg.ascii_only,
              ban_cr=cfg.ban_cr, max_run_length=cfg.max_run_length)
    compared = 0
    for _ in range(cfg.max_new):
        with torch.no_grad():
            row = model(torch.tensor([ctx[-cfg.seq_len:]]))[0, -1].numpy()
        u = torch.rand(1, generator=gen).numpy()
        i, _, mp, mu = sc.restate_row(row, ctx[-cfg.repetition_window:], u[0], **kw)
        if not (mp > sc.MARGIN and mu > sc.MARGIN):
            break                                                         # past a row inside the margin the texts may part
        assert text.encode()[len(ctx)] == i, (len(ctx), i)
        ctx.append(i)
        compared += 1
    assert compared >= 10                                                 # (all 12 with these seeds)
    assert text.encode()[len(prompt)] != ord("e")                         # the run of six bans a seventh
    with pytest.raises(ValueError, match="repetition_window"):
        pkg.generate(model, "a", pkg.SampleConfig(seq_len=64, repetition_window=0))
    with pytest.raises(ValueError, match="max_run_length"):
        pkg.generate(model, "a", pkg.SampleConfig(seq_len=64, repetition_window=4, max_run_length=6))
    assert pkg.generate(model, "", pkg.SampleConfig(seq_len=64, max_new=0)) == " "


@pytest.mark.parametrize("use_ema", [False, True])
def test_generate_chunked_native_sampler_is_the_torch_one_where_both_are_greedy(use_ema):
    import tensor_cuda_fft_amd as pkg
    z = fixture("X01_stream_2x48x32_k8_c4")
    torch.manual_seed(3)
    model = pkg.ChunkLM(build(z), 4, use_ema=use_ema, ema_chunk_len=16).eval()
    with torch.no_grad():
        model.head.weight.normal_(0.0, 0.3)
    a = pkg.generate_chunked(model, b"Once upon a time", 5, top_p=1e-9, sampler="torch")
    b = pkg.generate_chunked(model, b"Once upon a time", 5, top_p=1e-9, sampler="native")
    assert a == b and len(b) == 48 + 5 * 4
    assert a == pkg.generate_chunked(model, b"Once upon a time", 5, top_p=1e-9)          # the default is the torch sampler
    with pytest.raises(ValueError, match="sampler"):
        pkg.generate_chunked(model, b"x", 1, sampler="numpy")
