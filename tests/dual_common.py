"""Shared by the dual-head tests and tests/golden/make_golden_dual.py: deterministic stand-ins for a BPE tokenizer (no
test may load a real one) and the byte rows of the token-id fixture.  and the K21 step through a package handed in.
Nothing here imports the package under test or the reference."""
import zlib

import numpy as np
import torch

from conftest import TOL_ACT, TOL_PARAM, rel_err

TOKEN_VOCAB = 50257


class StubTokenizer:
    """`encode(text, add_special_tokens=False)`: one token per whitespace-separated word, its id the word's CRC-32 folded
    into 1 .. 50256 (never 0, the ignored id)."""

    def encode(self, text, add_special_tokens=False):
        return [1 + zlib.crc32(w.encode("utf-8")) % (TOKEN_VOCAB - 1) for w in text.split()]


class OverTokenizer:
    """Three tokens per character: more tokens than positions for any row without blanks."""

    def encode(self, text, add_special_tokens=False):
        return [1 + (7 * i + ord(ch)) % (TOKEN_VOCAB - 1) for ch in text for i in range(3)]


class RaisingTokenizer:
    def encode(self, text, add_special_tokens=False):
        raise RuntimeError("the tokenizer failed")


TOKENIZERS = {"words": StubTokenizer, "over": OverTokenizer, "raising": RaisingTokenizer}

T_IDS = 32


def _row(b: bytes) -> list:
    assert len(b) <= T_IDS
    return list(b.ljust(T_IDS, b" "))


def token_id_rows():
    """name -> (tokenizer name, (B, 32) int64 byte rows): ordinary text, invalid UTF-8, a whitespace-only row, more
    tokens than positions, exactly one token, and a tokenizer that raises."""
    text = [_row(b"the cat sat on the mat"), _row(b"a bb ccc dddd eeeee ffffff"), _row(b"one two three four five six7"),
            _row(b"  leading and trailing  ")]
    invalid = [_row(b"caf\xc3\xa9 \xff\xfe na\xc3 ve \x80 end"), _row(b"\xff\xff\xff"), _row("žluťoučký kůň".encode("utf-8"))]
    blank = [_row(b""), _row(b"\t\n \r"), _row(b"word after blank rows")]
    one = [_row(b"single"), _row(b"     x"), [ord("y")] * T_IDS]
    many = [[ord("a") + i % 26 for i in range(T_IDS)], _row(b"ab cd ef gh ij kl mn op qr st uv")]
    rows = {"text": ("words", text), "invalid_utf8": ("words", invalid), "blank": ("words", blank),
            "one_token": ("words", one), "many_tokens": ("over", many),
            "raising": ("raising", text[:2] + blank[:1])}
    return {k: (tok, np.array(v, np.int64)) for k, (tok, v) in rows.items()}


def stub_token_targets(x: torch.Tensor) -> torch.Tensor:
    """Token targets of a byte batch with the closed form of get_token_ids_fast over StubTokenizer, on the host: what a
    training-step test feeds the loss without going through the function under test."""
    B, T = x.shape
    out = torch.zeros((B, T), dtype=torch.int64)
    tok = StubTokenizer()
    for b, row in enumerate(x.cpu().tolist()):
        ids = tok.encode(bytes(row).decode("utf-8", errors="ignore"))
        if not ids:
            continue
        c = T // len(ids)
        for p in range(T):
            out[b, p] = ids[-1] if c == 0 else ids[min(p // c, len(ids) - 1)]
    return out.to(x.device)


def _t(a, device=None):
    out = torch.from_numpy(np.ascontiguousarray(a))
    return out if device is None else out.to(device)


def load_head(pkg, z):
    head = pkg.DualHead(int(z["d_model"]), vocab_size=256, token_vocab_size=int(z["token_vocab"]))
    head.load_state_dict({k[3:]: _t(v) for k, v in z.items() if k.startswith("sd.")}, strict=True)
    return head


def run_k21(pkg, z, device=None):
    """the K21 step through the package: name -> tensor, in the fixture's keys"""
    head = load_head(pkg, z).to(device or "cpu")
    h = _t(z["hidden"], device).requires_grad_(True)
    char_logits, token_logits = head(h)
    total, char_l, tok_l = pkg.compute_dual_loss(char_logits, token_logits, _t(z["y_char"], device),
                                                 _t(z["y_token"], device))
    total.backward()
    got = {"char_logits": char_logits, "loss_total": total, "loss_char": char_l, "loss_token": tok_l, "grad.hidden": h.grad}
    got.update({"grad." + k: p.grad for k, p in head.named_parameters()})
    return got, (char_l, tok_l)


def check_k21(got, z):
    for k, v in got.items():
        tol = TOL_PARAM if k.startswith("grad.") and k != "grad.hidden" else TOL_ACT
        assert float(z["ref_err_" + k]) <= tol / 4
        assert rel_err(v.detach().cpu().numpy(), z[k]) <= tol, k
