#!/usr/bin/env python3
"""Golden vectors of the word-structure heads, produced by the REFERENCE on CPU: generate_phase_targets and
PhaseClockChunkLM / compute_phase_clock_loss (fft_lm/phase_clock.py:68-213), get_word_boundaries and SegmentedChunkLM /
compute_segmented_loss (fft_lm/segmentation_head.py:58-196).

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_heads.py

K01: bytes and both target tensors for a (2, 1024) slice of the reference's data/valid.txt, a (3, 257) uniform block and
the short edge rows of tests/heads_common.py.  The generator FAILS unless the reference's labels equal the closed form of
heads_common.py exactly and its phase targets lie within a quarter of TOL_ACT of it (they are 2e-7 away: the reference's
fp32 linspace).
K11 / K12: the two models over heads_common.StubBackbone, d_model 32, (B, T) = (2, 48), chunk 4, with NON-ZERO head
weights (the reference's zero init would make parity vacuous): state_dict, x, both outputs, the three losses, and the
gradients of the total loss in every head parameter and in the hidden states.  Beside each fp32 result `ref_err_<key>`:
its max-normalised error against the same module in fp64, which must stay within a quarter of the tests' tolerance.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                     # noqa: E402  (puts the reference on sys.path)
from make_golden import SEED, REF                            # noqa: E402
import heads_common as hc                                    # noqa: E402
from conftest import TOL_ACT, TOL_PARAM, rel_err             # noqa: E402

from fft_lm.phase_clock import PhaseClockChunkLM, compute_phase_clock_loss, generate_phase_targets       # noqa: E402
from fft_lm.segmentation_head import SegmentedChunkLM, compute_segmented_loss, get_word_boundaries       # noqa: E402


def targets_case(name):
    corpus = np.frombuffer(open(os.path.join(REF, "data", "valid.txt"), "rb").read(), np.uint8)
    text = corpus[4096:4096 + 2048].reshape(2, 1024).astype(np.int64)
    rnd = np.random.default_rng(SEED).integers(0, 256, (3, 257)).astype(np.int64)
    rec = {}
    for key, x in (("text", text), ("random", rnd), ("edge", hc.edge_rows())):
        xt = torch.from_numpy(x)
        phase, bd = generate_phase_targets(xt), get_word_boundaries(xt)
        assert phase.dtype == torch.float32 and bd.dtype == torch.float32
        assert np.array_equal(bd.numpy(), hc.boundary_closed_form(x)), key
        e = rel_err(phase.numpy(), hc.phase_closed_form(x))
        assert e <= TOL_ACT / 4, (key, e)
        rec.update({key + ".x": x, key + ".phase": phase, key + ".boundary": bd, key + ".ref_err_phase": np.float64(e)})
    mg.save(name, rec)


def _tol(key):
    return TOL_PARAM if key.startswith("grad.") and key != "grad.hidden" else TOL_ACT


def model_case(name, cls, loss_fn, target_fn, head, B=2, T=48, chunk=4, d_model=32):
    torch.manual_seed(SEED)
    model = cls(hc.StubBackbone(d_model), chunk)
    with torch.no_grad():
        getattr(model, head).head.weight.normal_(0.0, 0.3)
        getattr(model, head).head.bias.normal_(0.0, 0.1)
    model.train()
    x = torch.from_numpy(np.random.default_rng(SEED).choice(
        np.array([32, 46, 10, 91, 125] + list(range(97, 123))), (B, T)).astype(np.int64))
    y_char = torch.randint(0, 256, (B, chunk))
    aux_t = target_fn(x)

    def run(m, dt):
        m.zero_grad()
        logits, aux = m(x)
        total, char_l, aux_l = loss_fn(logits, aux, y_char, aux_t.to(dt))
        total.backward()
        out = {"char_logits": logits.detach(), "aux": aux.detach(), "loss_total": total.detach(),
               "loss_char": char_l.detach(), "loss_aux": aux_l.detach(), "grad.hidden": m.backbone.last_hidden.grad}
        for k, p in m.named_parameters():
            if not k.startswith("backbone."):
                out["grad." + k] = p.grad
        return out

    m64 = copy.deepcopy(model).double()
    rec = run(model, torch.float32)
    ref64 = run(m64, torch.float64)
    for k, v in ref64.items():
        e = rel_err(rec[k].numpy(), v.numpy())
        assert e <= _tol(k) / 4, (name, k, e)
        rec["ref_err_" + k] = np.float64(e)
    assert float(rec["grad." + head + ".head.weight"].abs().max()) > 0
    rec.update({"x": x, "y_char": y_char, "aux_targets": aux_t, "chunk": np.int64(chunk), "d_model": np.int64(d_model),
                "keys": np.array(sorted(model.state_dict()))})
    for k, v in model.state_dict().items():
        rec["sd." + k] = v
    mg.save(name, rec)


if __name__ == "__main__":
    targets_case("K01_word_targets")
    model_case("K11_phaseclock_2x48x32", PhaseClockChunkLM, compute_phase_clock_loss, generate_phase_targets, "phase_head")
    model_case("K12_segmented_2x48x32", SegmentedChunkLM, compute_segmented_loss, get_word_boundaries, "seg_head")
