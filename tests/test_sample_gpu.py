"""The byte sampler on the GPU: smx_sample_bytes through functional.sample_bytes against the fp64 restatement
(tests/sample_common.py) and the reference's recorded rows (tests/golden/Y01_sample_rows.npz) under the rules of
test_sample_cpu.check_rows; reproducibility; a fixed-seed distribution check; the refusals; generate_chunked with the
native sampler, eager and from one captured graph; fixed_spectral.generate against its own CPU run.

Every body takes the device as an argument, so the same data can be walked on the CPU fallback (the shares the margin
rule leaves out depend on the data alone)."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden
import sample_common as sc
from tensor_cuda_fft_amd.functional import sample_bytes
from test_sample_cpu import check_rows, tiny_lm
from test_stream_cpu import build, fixture

pytestmark = pytest.mark.gpu

STRIDE = 320                # floats between two rows of logits: the rows are read in place
DIST_ROWS = 65536


def run_strided(logits, recent, u, dev, **kw):
    """sample_bytes on rows that lie STRIDE floats apart (a view: nothing is copied on the way in)."""
    base = torch.full((logits.shape[0], STRIDE), float("nan"), device=dev)
    base[:, :256] = torch.from_numpy(logits).to(dev)
    x = base[:, :256]
    assert x.stride(0) == STRIDE or x.shape[0] == 1
    ids, p = sample_bytes(x, torch.from_numpy(np.asarray(recent)).to(dev), torch.from_numpy(u).to(dev), return_probs=True,
                          **kw)
    return ids.cpu().numpy(), p.cpu().numpy()


def body_switches(dev, name, R):
    kw = sc.SETTINGS[name]
    logits, u = sc.make_rows(R, 40)          # (with this seed the restatement leaves out 0, 1 of 16 and 3 of 67 rows at most)
    recent = sc.make_window(256, 50, run=6 if "max_run_length" in kw else 0)
    ids, p = run_strided(logits, recent, u, dev, **kw)
    check_rows(ids, p, logits, recent, u, kw, what=f"{name} R={R}")


def body_windows(dev, n, dtype):
    kw = sc.SETTINGS["all"]
    logits, u = sc.make_rows(16, 60)
    recent = sc.make_window(n, 70 + n, run=6 if n >= 6 else 0).astype(dtype)
    ids, p = run_strided(logits, recent, u, dev, **kw)
    check_rows(ids, p, logits, recent, u, kw, what=f"n_recent {n} {np.dtype(dtype).name}")


def body_fixture(dev):
    z = load_golden("Y01_sample_rows")
    for c in z["cases"].tolist():
        kw = json.loads(str(z[c + ".settings"]))
        ids, p = run_strided(z[c + ".logits"], z[c + ".recent"], z[c + ".u"], dev, **kw)
        ref = z[c + ".probs"]
        assert np.array_equal(p > 0, ref > 0), c
        assert np.abs(p - ref).max() <= 1e-5, c
        check_rows(ids, p, z[c + ".logits"], z[c + ".recent"], z[c + ".u"], kw, what=c)


def body_distribution(dev):
    """One distribution, DIST_ROWS draws from seeded uniforms: every byte's frequency within 5 standard deviations of its
    probability (a byte of probability 0 never)."""
    kw = sc.SETTINGS["all"]
    logits, _ = sc.make_rows(1, 80, scale=1.0)                   # a flat row: some dozens of bytes stay in the nucleus
    recent = sc.make_window(256, 81)
    u = torch.rand(DIST_ROWS, generator=torch.Generator().manual_seed(82)).to(dev)       # the same on every device
    rows = torch.from_numpy(logits).to(dev).expand(DIST_ROWS, 256)
    ids, p = sample_bytes(rows, torch.from_numpy(recent).to(dev), u, return_probs=True, **kw)
    assert torch.equal(p, p[:1].expand_as(p))                                            # a row does not depend on the others
    p0 = p[0].double().cpu().numpy()
    freq = np.bincount(ids.cpu().numpy(), minlength=256) / DIST_ROWS
    sd = np.sqrt(p0 * (1 - p0) / DIST_ROWS)
    z = np.abs(freq - p0) / np.where(sd > 0, sd, 1.0)
    print(f"{int((p0 > 0).sum())} bytes can be drawn, smallest p {p0[p0 > 0].min():.3e}, largest deviation {z.max():.2f} sd")
    assert (freq[p0 == 0] == 0).all() and z.max() <= 5.0
    assert (p0 > 0).sum() >= 5 and abs(p0.sum() - 1) < 1e-5


@pytest.mark.parametrize("R", [1, 16, 67])
@pytest.mark.parametrize("name", sorted(sc.SETTINGS))
def test_native_equals_the_restatement_switch_by_switch(gpu, name, R):
    body_switches(gpu, name, R)


@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4096])
def test_native_windows(gpu, n, dtype):
    body_windows(gpu, n, dtype)


def test_native_equals_the_reference_rows(gpu):
    body_fixture(gpu)


def test_native_distribution(gpu):
    body_distribution(gpu)


def test_runs_are_bitwise_equal_and_rows_do_not_interact(gpu):
    kw = sc.SETTINGS["all"]
    logits, u = sc.make_rows(67, 90)
    recent = sc.make_window(300, 91, run=6)
    ids, p = run_strided(logits, recent, u, gpu, **kw)
    ids2, p2 = run_strided(logits, recent, u, gpu, **kw)
    assert np.array_equal(ids, ids2) and np.array_equal(p.view(np.uint32), p2.view(np.uint32))
    for r in (0, 1, 33, 66):
        i1, p1 = run_strided(logits[r:r + 1], recent, u[r:r + 1], gpu, **kw)
        assert i1[0] == ids[r] and np.array_equal(p1[0].view(np.uint32), p[r].view(np.uint32)), r
    # without probs the ids are the same; u=None draws from the device's generator, reproducibly
    x, w = torch.from_numpy(logits).to(gpu), torch.from_numpy(recent).to(gpu)
    assert np.array_equal(sample_bytes(x, w, torch.from_numpy(u).to(gpu), **kw).cpu().numpy(), ids)
    g = lambda: torch.Generator(device=gpu).manual_seed(5)
    assert torch.equal(sample_bytes(x, w, generator=g(), **kw), sample_bytes(x, w, generator=g(), **kw))


def test_edge_rows_never_fault_and_never_draw_probability_zero(gpu):
    logits = np.full((3, 256), -np.inf, np.float32)
    logits[:, 65:68] = 0.0
    logits[2, 3] = np.nan
    e = np.zeros(0, np.int64)
    ids, p = run_strided(logits, e, np.array([0.99999994, 0.0, 0.5], np.float32), gpu)
    assert ids[:2].tolist() == [67, 65] and (p[:2, 68:] == 0).all() and 0 <= ids[2] <= 255
    ids, _ = run_strided(logits, e, np.array([np.nan, 1.5, 0.5], np.float32), gpu, top_p=0.9, top_k=3)
    assert ids[0] in (65, 66) and ids[1] == 66 and 0 <= ids[2] <= 255
    ids, p = run_strided(np.zeros((1, 256), np.float32), e, np.array([0.5], np.float32), gpu, top_p=3.5 / 256)
    assert np.flatnonzero(p[0]).tolist() == [0, 1, 2] and ids[0] == 1                    # equal logits: by index


def test_refusals_enqueue_nothing(gpu):
    from tensor_cuda_fft_amd import _lib
    lib = _lib.lib()
    logits = torch.zeros(4, 256, device=gpu)
    recent = torch.zeros(8, dtype=torch.int64, device=gpu)
    u = torch.full((4,), 0.5, device=gpu)
    ids = torch.full((4,), -7, dtype=torch.int64, device=gpu)
    probs = torch.full((4, 256), -7.0, device=gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream

    def call(lg=logits.data_ptr(), stride=256, tb=8, temp=0.8, V=256, out=ids.data_ptr()):
        return lib.smx_sample_bytes(lg, stride, recent.data_ptr(), tb, 8, temp, 0.9, 0, 1.25, 0.0, 0.0, 1, 1, 6,
                                    u.data_ptr(), out, probs.data_ptr(), 4, V, stream)

    assert call(V=255) == -2                                              # SMX_ERR_UNSUPPORTED
    assert call(temp=0.0) == -1 and call(lg=None) == -1 and call(out=None) == -1 and call(tb=4) == -1 \
        and call(stride=255) == -1                                        # SMX_ERR_INVALID
    torch.cuda.synchronize(gpu)
    assert (ids == -7).all() and (probs == -7.0).all()                    # nothing ran
    assert call() == 0
    torch.cuda.synchronize(gpu)
    assert ((ids >= 0) & (ids <= 255)).all() and (probs >= 0).all()


def chunk_model(gpu):
    import tensor_cuda_fft_amd as pkg
    z = fixture("X01_stream_2x48x32_k8_c4")
    torch.manual_seed(3)
    model = pkg.ChunkLM(build(z), 4, use_ema=True, ema_chunk_len=16).eval()
    with torch.no_grad():
        model.head.weight.normal_(0.0, 0.3)
    return model.to(gpu)


def test_generate_chunked_native_sampler_eager_and_from_a_graph(gpu):
    import tensor_cuda_fft_amd as pkg
    model = chunk_model(gpu)
    a = pkg.generate_chunked(model, b"Once upon a time", 6, top_p=1e-9, sampler="torch")
    b = pkg.generate_chunked(model, b"Once upon a time", 6, top_p=1e-9, sampler="native")
    c = pkg.generate_chunked(model, b"Once upon a time", 6, top_p=1e-9, sampler="native", use_graph=True)
    assert a == b == c and len(a) == 48 + 6 * 4 and a[:48] == b" " * 32 + b"Once upon a time"
    # a real nucleus and a seeded generator: the graph draws what the eager loop draws
    g = lambda: torch.Generator(device=gpu).manual_seed(17)
    d = pkg.generate_chunked(model, b"Once upon a time", 6, top_p=0.9, sampler="native", generator=g())
    e = pkg.generate_chunked(model, b"Once upon a time", 6, top_p=0.9, sampler="native", generator=g(), use_graph=True)
    assert d == e and len(d) == 48 + 6 * 4
    assert d != pkg.generate_chunked(model, b"Once upon a time", 6, top_p=0.9, sampler="native",
                                     generator=torch.Generator(device=gpu).manual_seed(18))   # (the seed matters)
    torch.manual_seed(23)                                                 # ... and with the device's default generator
    f = pkg.generate_chunked(model, b"Once upon a time", 6, top_p=0.9, sampler="native")
    torch.manual_seed(23)
    assert f == pkg.generate_chunked(model, b"Once upon a time", 6, top_p=0.9, sampler="native", use_graph=True)


def test_generate_on_the_gpu_equals_its_cpu_run_on_the_same_uniforms(gpu, monkeypatch):
    import tensor_cuda_fft_amd as pkg
    cfg = pkg.SampleConfig(seq_len=64, max_new=12)
    prompt = "Once upon a time there was a spectral model that read bytes, one by one: " + "e" * 6
    us = torch.rand(cfg.max_new, generator=torch.Generator().manual_seed(11))
    real = torch.rand

    def texts(model):
        it = iter(us)
        monkeypatch.setattr(torch, "rand", lambda *a, device=None, **k: next(it).reshape(1).to(device))
        try:
            return pkg.generate(model, prompt, cfg).encode()
        finally:
            monkeypatch.setattr(torch, "rand", real)

    model = tiny_lm()
    on_cpu = texts(model)
    on_gpu = texts(model.to(gpu))
    model = model.cpu()
    # how far the CPU text is comparable: the restatement along it
    kw = dict(temperature=cfg.temperature, top_p=cfg.top_p, top_k=cfg.top_k, repetition_penalty=cfg.repetition_penalty,
              presence_penalty=cfg.presence_penalty, frequency_penalty=cfg.frequency_penalty, ascii_only=cfg.ascii_only,
              ban_cr=cfg.ban_cr, max_run_length=cfg.max_run_length)
    n0, upto = len(prompt), len(prompt)
    for k in range(cfg.max_new):
        ctx = list(on_cpu[:n0 + k])
        with torch.no_grad():
            row = model(torch.tensor([ctx[-cfg.seq_len:]]))[0, -1].numpy()
        i, _, mp, mu = sc.restate_row(row, ctx[-cfg.repetition_window:], float(us[k]), **kw)
        if not (mp > sc.MARGIN and mu > sc.MARGIN):
            break
        assert on_cpu[n0 + k] == i
        upto = n0 + k + 1
    print(f"{upto - n0} of {cfg.max_new} bytes comparable")
    assert upto - n0 >= 6 and on_gpu[:upto] == on_cpu[:upto] and len(on_gpu) == n0 + cfg.max_new
