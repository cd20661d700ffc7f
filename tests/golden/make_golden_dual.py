#!/usr/bin/env python3
"""Golden vectors of the dual head, produced by the REFERENCE on CPU: DualHead / compute_dual_loss and get_token_ids_fast
(fft_lm/dual_head.py:29-193), and the state_dict keys of its TokenAwareChunkLM.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dual.py

K21: DualHead(d_model=8, vocab_size=256, token_vocab_size=4099) on a (2, 24, 8) hidden state with compute_dual_loss:
state_dict, inputs, both target tensors (the token targets hold zeros, the ignored positions), the three losses and the
gradients of the total loss in the hidden state and the four parameters.  Beside each fp32 result `ref_err_<key>`: its
max-normalised error against the same module in fp64, which must stay within a quarter of the tests' tolerance.
K22: get_token_ids_fast over the rows of tests/dual_common.py with its stand-in tokenizers (no real tokenizer is ever
loaded), and the sorted state_dict keys of a reference TokenAwareChunkLM over heads_common.StubBackbone (the 50257-row
weight itself is not stored).
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
from make_golden import SEED                                 # noqa: E402
import dual_common as dc                                     # noqa: E402
import heads_common as hc                                    # noqa: E402
from conftest import TOL_ACT, TOL_PARAM, rel_err             # noqa: E402

from fft_lm.dual_head import DualHead, TokenAwareChunkLM, compute_dual_loss, get_token_ids_fast       # noqa: E402


def _tol(key):
    return TOL_PARAM if key.startswith("grad.") and key != "grad.hidden" else TOL_ACT


def loss_case(name, B=2, T=24, d_model=8, token_vocab=4099):
    torch.manual_seed(SEED)
    head = DualHead(d_model, vocab_size=256, token_vocab_size=token_vocab)
    with torch.no_grad():                                     # logits of order 1: the 0.02 init would make every row flat
        head.char_head.weight.normal_(0.0, 0.5)
        head.token_head.weight.normal_(0.0, 0.5)
        head.char_head.bias.normal_(0.0, 0.1)
        head.token_head.bias.normal_(0.0, 0.1)
    hidden = torch.randn(B, T, d_model)
    y_char = torch.randint(0, 256, (B, T))
    y_tok = torch.randint(1, token_vocab, (B, T))
    y_tok[0, :5] = 0                                          # ignored positions
    y_tok[1, 7::6] = 0
    y_tok[1, -1] = token_vocab - 1

    def run(m, dt):
        m.zero_grad()
        h = hidden.detach().clone().to(dt).requires_grad_(True)
        char_logits, token_logits = m(h)
        total, char_l, tok_l = compute_dual_loss(char_logits, token_logits, y_char, y_tok)
        total.backward()
        out = {"char_logits": char_logits.detach(), "token_logits": token_logits.detach(), "loss_total": total.detach(),
               "loss_char": char_l.detach(), "loss_token": tok_l.detach(), "grad.hidden": h.grad}
        out.update({"grad." + k: p.grad for k, p in m.named_parameters()})
        return out

    rec = run(head, torch.float32)
    ref64 = run(copy.deepcopy(head).double(), torch.float64)
    for k, v in ref64.items():
        e = rel_err(rec[k].numpy(), v.numpy())
        assert e <= _tol(k) / 4, (name, k, e)
        rec["ref_err_" + k] = np.float64(e)
    del rec["token_logits"]                                   # 0.8 MB; the losses and gradients carry it
    rec.update({"hidden": hidden, "y_char": y_char, "y_token": y_tok, "d_model": np.int64(d_model),
                "token_vocab": np.int64(token_vocab)})
    for k, v in head.state_dict().items():
        rec["sd." + k] = v
    mg.save(name, rec)


def token_ids_case(name):
    rec = {}
    for key, (tok, x) in dc.token_id_rows().items():
        ids = get_token_ids_fast(torch.from_numpy(x), dc.TOKENIZERS[tok]())
        assert ids.shape == x.shape and ids.dtype == torch.int64
        rec.update({key + ".x": x, key + ".ids": ids, key + ".tokenizer": np.array(tok)})
    assert not rec["blank.ids"][:2].any() and rec["blank.ids"][2].all()
    assert (rec["raising.ids"][:2].numpy() == 220).all() and not rec["raising.ids"][2].any()   # a blank row is never encoded
    over = rec["many_tokens.ids"].numpy()
    assert (over == over[:, -1:]).all()                       # n > T: the whole row holds the last token
    model = TokenAwareChunkLM(hc.StubBackbone(8), 4)
    rec["keys"] = np.array(sorted(model.state_dict()))
    mg.save(name, rec)


if __name__ == "__main__":
    loss_case("K21_dual_loss")
    token_ids_case("K22_token_ids")
