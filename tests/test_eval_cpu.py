"""What the trainer runs at the end of an epoch, without a GPU: find_snippets on the host route against bytes.find,
parroting_score / eval_loss / load_state_flexible against the reference's recorded results (V01, V02, V03), the corpus
loader, the checkpoint files, and the argument checks of the smx_match_* entries."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import eval_common as ec
from conftest import ROOT, TOL_ACT, load_golden, rel_err

NAMES = ("find_snippets", "load_corpus_as_u8", "eval_loss", "parroting_score", "save_checkpoint", "verify_checkpoint",
         "load_checkpoint", "checkpoint_state", "config_from_checkpoint", "load_state_flexible")


def pkg():
    import tensor_cuda_fft_amd
    return tensor_cuda_fft_amd


@pytest.fixture(scope="module")
def L():
    """the ctypes binding, with libsmx.so built first on a fresh checkout (as tests/test_abi.py does)"""
    from tensor_cuda_fft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "tensor-cuda-fft-_amd", "csrc", "build.sh")], check=True,
                       capture_output=True)
    return _lib


def test_names_are_exported():
    p = pkg()
    for n in NAMES:
        assert n in p.__all__ and hasattr(p, n), n
    assert "Out of scope: the CLIs and the optimizer" in " ".join(p.training.__doc__.split())


# ---- find_snippets on the host route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_", [4, 64, 256])
def test_find_snippets_on_cpu_tensors_and_bytes_is_bytes_find(L_):
    p = pkg()
    n = 3000
    corpus = ec.random_corpus(n, 7 + L_, 0, 200)
    corpus[1200:1200 + L_] = corpus[500:500 + L_]                    # a repeated occurrence: the first one counts
    blob = bytes(corpus.numpy().tobytes())
    cut = torch.cat([corpus[n - L_ // 2:], torch.full((L_,), 250, dtype=torch.uint8)])[:L_]
    snips = torch.stack([corpus[:L_], corpus[n - L_:], cut, corpus[500:500 + L_], corpus[1200:1200 + L_],
                         corpus[:L_].clone(), torch.full((L_,), 222, dtype=torch.uint8)])
    want = ec.find_all(blob, snips)
    assert want[0] == 0 and want[1] == n - L_ and want[2] == -1 and want[6] == -1
    assert 0 <= want[3] <= 500 and want[4] == want[3] and want[5] == 0          # the first occurrence; duplicates
    for c in (corpus, blob):
        got = p.find_snippets(c, snips)
        assert got.dtype == torch.int64 and got.shape == (7,) and torch.equal(got, want)
    assert torch.equal(p.find_snippets(corpus[:L_ - 1], snips), torch.full((7,), -1))      # n < L
    assert torch.equal(p.find_snippets(b"", snips), torch.full((7,), -1))
    assert torch.equal(p.find_snippets(corpus[::2], snips), ec.find_all(bytes(corpus[::2].tolist()), snips))


def test_find_snippets_checks_its_arguments():
    p = pkg()
    corpus = ec.random_corpus(100, 1)
    snips = corpus[:8].view(1, 8)
    assert p.find_snippets(corpus, snips[:0]).shape == (0,)
    for bad in (corpus.long(), corpus.view(10, 10), [1, 2, 3]):
        with pytest.raises(TypeError):
            p.find_snippets(bad, snips)
    for bad in (snips.long(), snips[0], b"abcd"):
        with pytest.raises(TypeError):
            p.find_snippets(corpus, bad)
    with pytest.raises(ValueError):
        p.find_snippets(corpus, snips, max_workgroups=-1)


# ---- parroting_score against the reference's recorded picks and scores ---------------------------------------------------------
@pytest.fixture(scope="module")
def parrot():
    return load_golden("V01_parroting")


def test_parroting_score_equals_the_reference_exactly(parrot):
    p = pkg()
    cfg = p.TrainConfig()
    blob = bytes(parrot["corpus"].tobytes())
    tensor = torch.from_numpy(parrot["corpus"].copy())
    scores = set()
    for g in parrot["names"]:
        gen = bytes(parrot[f"{g}.gen"].tobytes())
        picks = p.parroting_picks(len(gen), cfg)
        assert picks.dtype == np.int64 and np.array_equal(picks, parrot[f"{g}.picks"]), g
        for corpus in (blob, tensor):
            got = p.parroting_score(corpus, gen, cfg)
            assert isinstance(got, float) and got == float(parrot[f"{g}.score"]), g
        scores.add(got)
    assert len(scores) >= 4 and {0.0, 1.0} <= scores


def test_parroting_score_makes_one_search_call(parrot, monkeypatch):
    p = pkg()
    calls = []
    real = p.training.find_snippets
    monkeypatch.setattr(p.training, "find_snippets", lambda c, s: calls.append(tuple(s.shape)) or real(c, s))
    gen = bytes(parrot["mixed2000.gen"].tobytes())
    assert p.parroting_score(bytes(parrot["corpus"].tobytes()), gen, p.TrainConfig()) == float(parrot["mixed2000.score"])
    assert calls == [(64, 64)]
    assert p.parroting_score(b"", gen[:64], p.TrainConfig()) == 0.0 and len(calls) == 1        # the early return


# ---- eval_loss on the CPU route ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lossfix():
    return load_golden("V02_eval_loss")


@pytest.mark.parametrize("geom", ec.GEOMETRIES)
def test_eval_loss_on_the_cpu_matches_the_reference(lossfix, geom):
    p = pkg()
    z = lossfix
    model, cfg, starts = ec.load_lm(p, z, geom)
    corpus = torch.from_numpy(z["corpus"].copy())
    model.train()
    for cname, cutoff in (("none", None), ("cut", int(z[geom + ".cutoff"]))):
        assert float(z[f"{geom}.ref_err_{cname}"]) <= TOL_ACT / 4
        torch.manual_seed(int(z["seed"]))
        got = p.eval_loss(model, corpus, starts, cfg, cutoff)
        after = torch.get_rng_state()
        e = rel_err(np.float64(got), z[f"{geom}.loss64.{cname}"])
        print(f"{geom} cutoff={cutoff}: loss {got!r} reference {float(z[f'{geom}.loss64.{cname}'])!r} rel_err {e:.3g}")
        assert isinstance(got, float) and e <= TOL_ACT
        assert not model.training                                    # left in eval mode, as the reference leaves it
        torch.manual_seed(int(z["seed"]))
        torch.randperm(starts.numel())
        assert torch.equal(after, torch.get_rng_state())             # exactly one randperm draw from the global generator


def test_eval_loss_without_a_full_batch_is_zero(lossfix):
    p = pkg()
    model, cfg, starts = ec.load_lm(p, lossfix, "filter")
    corpus = torch.from_numpy(lossfix["corpus"].copy())
    assert p.eval_loss(model, corpus, starts[:1], cfg, None) == 0.0
    assert p.eval_loss(model, corpus, starts[:0], cfg, None) == 0.0
    torch.manual_seed(5)
    three = p.eval_loss(model, corpus, starts[:3], cfg, None)       # one full batch of two; the odd window is dropped
    torch.manual_seed(5)
    sel = starts[:3][torch.randperm(3)][:2]
    x, y = p.sample_windows(corpus, sel, cfg.seq_len)
    with torch.no_grad():
        want = torch.nn.functional.cross_entropy(model(x).reshape(-1, 256), y.reshape(-1))
    assert rel_err(np.float64(three), np.float64(want.item())) <= TOL_ACT


# ---- corpus loader, checkpoints -----------------------------------------------------------------------------------------------
def test_load_corpus_as_u8(tmp_path):
    p = pkg()
    path = tmp_path / "corpus.bin"
    path.write_bytes(bytes(range(256)) + b"two\nlines\r\n")
    raw = p.load_corpus_as_u8(str(path), sanitize_ascii=False)
    assert raw.dtype == torch.uint8 and raw.dim() == 1 and bytes(raw.tolist()) == path.read_bytes()
    clean = p.load_corpus_as_u8(str(path), sanitize_ascii=True)
    want = bytes(b if b == 10 or 32 <= b <= 126 else 32 for b in path.read_bytes())
    assert clean.dtype == torch.uint8 and bytes(clean.tolist()) == want and clean.is_contiguous()
    assert p.load_corpus_as_u8(str(path), sanitize_ascii=True, device="cpu").device.type == "cpu"
    raw[0] = 9                                                       # owns its memory


def test_checkpoint_round_trip_and_integrity(tmp_path):
    p = pkg()
    cfg = p.TrainConfig(d_model=16, n_layers=1, seq_len=32, kernel_len=8, amp=False)
    model = p.FixedSpectralLM(cfg)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    state = p.checkpoint_state(model, opt, None, cfg, 7)
    assert list(state) == ["epoch", "model", "opt", "scaler", "cfg"]             # the reference's keys, in its order
    assert state["epoch"] == 7 and state["scaler"] is None and state["cfg"]["seq_len"] == 32
    assert sorted(state["model"]) == sorted(model.state_dict()) and "param_groups" in state["opt"]
    assert p.checkpoint_state(model, None, None, cfg, 0)["opt"] is None
    path = str(tmp_path / "sub" / "ckpt.pt")
    p.save_checkpoint(state, path)
    digest = open(path + ".sha256").read()
    assert len(digest.strip()) == 64 and digest.endswith("\n")
    assert p.verify_checkpoint(path) is True
    back = p.load_checkpoint(path)
    assert back["epoch"] == 7 and back["cfg"] == state["cfg"]
    assert all(torch.equal(back["model"][k], v) for k, v in model.state_dict().items())
    with open(path, "ab") as f:                                     # tampered
        f.write(b"x")
    with pytest.raises(RuntimeError) as err:
        p.load_checkpoint(path)
    import hashlib
    actual = hashlib.sha256(open(path, "rb").read()).hexdigest()
    assert str(err.value) == (f"Checkpoint integrity check failed for {path}. "
                              f"Expected sha256={digest.strip()}, got sha256={actual}.")
    bare = str(tmp_path / "bare.pt")
    torch.save(state, bare)                                          # no sidecar: loads, and says it was not verified
    assert p.verify_checkpoint(bare) is False and p.load_checkpoint(bare)["epoch"] == 7


def test_config_from_checkpoint_merges_known_fields_only():
    p = pkg()
    ckpt = {"cfg": {"seq_len": 77, "d_model": 48, "no_such_field": 1}}
    cfg = p.config_from_checkpoint(ckpt)
    assert isinstance(cfg, p.TrainConfig) and (cfg.seq_len, cfg.d_model) == (77, 48) and not hasattr(cfg, "no_such_field")
    assert cfg.kernel_len == p.TrainConfig().kernel_len
    mine = p.TrainConfig(kernel_len=5)
    assert p.config_from_checkpoint(ckpt, mine) is mine and (mine.seq_len, mine.kernel_len) == (77, 5)
    assert p.config_from_checkpoint({"epoch": 1}).seq_len == 1024 and p.config_from_checkpoint({"cfg": None}).seq_len == 1024


def test_load_state_flexible_equals_the_reference():
    p = pkg()
    z = load_golden("V03_flexible")
    mk = lambda a: p.FixedSpectralLM(p.TrainConfig(d_model=int(a[0]), n_layers=int(a[1]), seq_len=int(a[2]),
                                                   kernel_len=int(a[3])))
    old, new = mk(z["old"]), mk(z["new"])
    with torch.no_grad():
        for blk in old.blocks:
            blk.gate_freq_logits.copy_(torch.arange(blk.gate_freq_logits.numel(), dtype=torch.float32))
    before = {k: v.clone() for k, v in new.state_dict().items()}
    state = dict(old.state_dict())
    state[str(z["unknown_key"])] = torch.zeros(3)
    resized, skipped = p.load_state_flexible(new, state)
    fmt = lambda rows: [f"{k} {tuple(a)} {tuple(b)}" for k, a, b in rows]
    assert fmt(resized) == list(z["resized"]) and fmt(skipped) == list(z["skipped"])
    now = new.state_dict()
    n_old = old.blocks[0].gate_freq_logits.numel()
    for i in range(2):
        g = now[f"blocks.{i}.gate_freq_logits"]
        assert torch.equal(g[:n_old], torch.arange(n_old, dtype=torch.float32)) and torch.equal(g[n_old:], before[f"blocks.{i}.gate_freq_logits"][n_old:])
        assert torch.equal(now[f"blocks.{i}.kernel"], before[f"blocks.{i}.kernel"])        # skipped: untouched
    assert torch.equal(now["embed.weight"], old.state_dict()["embed.weight"])             # same shape: loaded


# ---- the C entries' argument checks ---------------------------------------------------------------------------------------------
def test_match_entries_validate_without_touching_the_gpu(L):
    lib = L.lib()
    err = lambda: lib.smx_last_error().decode()
    assert [lib.smx_match_supported(s, l) for s, l in ((1, 4), (256, 128), (128, 256), (23, 64), (64, 64))] == [1] * 5
    assert [lib.smx_match_supported(s, l) for s, l in ((0, 64), (257, 4), (1, 3), (1, 257), (256, 129), (129, 256))] == [0] * 6
    n = ctypes.c_size_t()
    assert lib.smx_match_workspace_bytes(64, 64, ctypes.byref(n)) == 0 and n.value % 256 == 0 and n.value >= 64 * 8
    assert lib.smx_match_workspace_bytes(64, 64, None) == -1
    assert lib.smx_match_workspace_bytes(300, 64, ctypes.byref(n)) == -2 and "smx_match_supported" in err()
    lib.smx_match_workspace_bytes(2, 8, ctypes.byref(n))
    corpus = (ctypes.c_ubyte * 64)()
    snips = (ctypes.c_ubyte * 16)()
    first = (ctypes.c_longlong * 4)()
    ws = ctypes.create_string_buffer(n.value + 512)
    c, s, f = ctypes.addressof(corpus), ctypes.addressof(snips), ctypes.addressof(first)
    w = (ctypes.addressof(ws) + 255) // 256 * 256
    call = lambda *a: lib.smx_match_first(*a, None)
    assert call(c, 64, s, 2, 3, f, w, n.value, 0) == -2 and "S=2 L=3" in err()                 # unsupported set
    assert call(c, 64, s, 257, 8, f, w, n.value, 0) == -2
    assert call(c, -1, s, 2, 8, f, w, n.value, 0) == -1 and "negative" in err()
    assert call(None, 64, s, 2, 8, f, w, n.value, 0) == -1 and "non-NULL" in err()
    assert call(c, 64, None, 2, 8, f, w, n.value, 0) == -1 and "non-NULL" in err()
    assert call(c, 64, s, 2, 8, None, w, n.value, 0) == -1 and "non-NULL" in err()
    assert call(c, 64, s, 2, 8, f + 4, w, n.value, 0) == -1 and "8-byte aligned" in err()
    assert call(c, 64, s, 2, 8, f, w, n.value, -1) == -1 and "max_workgroups" in err()
    assert call(c, 64, s, 2, 8, f, None, 0, 0) == -4 and "workspace is NULL" in err()
    assert call(c, 64, s, 2, 8, f, w, n.value - 1, 0) == -4 and "workspace has" in err()
    assert call(c, 64, s, 2, 8, f, w + 8, n.value, 0) == -4 and "256-byte aligned" in err()
    assert set(("smx_match_supported", "smx_match_workspace_bytes", "smx_match_first")) <= set(L._SIGS)
    assert "train_fixed_full.py:185-205" in open(os.path.join(ROOT, "include", "smx.h")).read()
