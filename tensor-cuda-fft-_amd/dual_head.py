"""Drop-in for `fft_lm.dual_head`: multi-scale supervision, a 256-way character head (what generation uses) beside a
50257-way token head (a teacher signal during training, dropped afterwards).

The two `nn.Linear` heads stay in torch; the cross-entropy over their logits is the native row loss
(functional.cross_entropy): the (B, T, 50257) token logits are read once forward and once backward.  The token ids of a
byte batch come from the tokenizer on the host (by nature) and are spread over the positions with whole-tensor ops."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import functional as F_


class DualHead(nn.Module):
    """hidden (B, T, d_model) -> char logits (B, T, vocab_size) and, with `return_token_logits`, token logits
    (B, T, token_vocab_size).  Weights N(0, 0.02), biases zero."""

    def __init__(self, d_model: int, vocab_size: int = 256, token_vocab_size: int = 50257):
        super().__init__()
        self.d_model = d_model
        self.vocab_size = vocab_size
        self.token_vocab_size = token_vocab_size
        self.char_head = nn.Linear(d_model, vocab_size)
        self.token_head = nn.Linear(d_model, token_vocab_size)
        nn.init.normal_(self.char_head.weight, mean=0.0, std=0.02)
        nn.init.zeros_(self.char_head.bias)
        nn.init.normal_(self.token_head.weight, mean=0.0, std=0.02)
        nn.init.zeros_(self.token_head.bias)

    def forward(self, hidden: torch.Tensor, return_token_logits: bool = True):
        char_logits = self.char_head(hidden)
        if return_token_logits:
            return char_logits, self.token_head(hidden)
        return char_logits


def _decode(row) -> str:
    try:
        return bytes(row).decode("utf-8", errors="ignore")
    except Exception:                                   # values outside 0..255: one character per value
        return "".join(chr(c) for c in row)


def get_token_ids_fast(text_bytes: torch.Tensor, tokenizer) -> torch.Tensor:
    """Approximate token id of every byte position, (B, T) in the dtype and on the device of `text_bytes`: a row is
    decoded as UTF-8 (errors ignored) and tokenised by `tokenizer.encode(text, add_special_tokens=False)`; token i of n
    covers positions [i c, (i + 1) c) with c = T // n and the last token runs to T (so with n > T the whole row holds the
    last token).  A row that is empty or only whitespace, or that yields no token, stays 0; a tokenizer that raises
    fills the row with 220 (GPT-2's space)."""
    B, T = text_bytes.shape
    rows = text_bytes.cpu().tolist()
    lists = []
    for row in rows:                                    # the tokenizer runs on the host
        text = _decode(row)
        if not text.strip():
            lists.append([])
            continue
        try:
            lists.append([int(t) for t in tokenizer.encode(text, add_special_tokens=False)])
        except Exception:
            lists.append([220])
    n_max = max([len(t) for t in lists] + [1])
    dev = text_bytes.device
    padded = torch.tensor([t + [0] * (n_max - len(t)) for t in lists], dtype=torch.int64).reshape(B, n_max).to(dev)
    n = torch.tensor([len(t) for t in lists], dtype=torch.int64).reshape(B, 1).to(dev)
    last = (n - 1).clamp(min=0)
    c = T // n.clamp(min=1)                             # 0 where a row has more tokens than positions
    pos = torch.arange(T, device=dev).expand(B, T)
    which = torch.where(c > 0, torch.minimum(pos // c.clamp(min=1), last), last)
    return padded.gather(1, which).to(text_bytes.dtype)


def compute_dual_loss(char_logits: torch.Tensor, token_logits: torch.Tensor, char_targets: torch.Tensor,
                      token_targets: torch.Tensor, char_weight: float = 1.0, token_weight: float = 0.5):
    """(total, char_loss, token_loss): the mean cross-entropy of the 256-way char logits plus `token_weight` x that of
    the token logits, where a token target of 0 is ignored."""
    char_loss = F_.cross_entropy(char_logits.reshape(-1, 256), char_targets.reshape(-1), reduction="mean")
    token_loss = F_.cross_entropy(token_logits.reshape(-1, token_logits.size(-1)), token_targets.reshape(-1),
                                  ignore_index=0, reduction="mean")
    return char_weight * char_loss + token_weight * token_loss, char_loss, token_loss


class TokenAwareChunkLM(nn.Module):
    """`backbone` (with `cfg.d_model` and `forward_hidden(x, cutoff=...)`) plus the dual head: in training mode
    `(char_logits (B, chunk, 256), token_logits (B, T, 50257))`, in eval mode the char logits alone."""

    def __init__(self, backbone: nn.Module, chunk: int, tokenizer=None):
        super().__init__()
        self.backbone = backbone
        self.chunk = chunk
        self.tokenizer = tokenizer
        self.head = DualHead(backbone.cfg.d_model, vocab_size=256, token_vocab_size=50257)

    def forward(self, x: torch.Tensor, cutoff: Optional[int] = None, return_token_logits: Optional[bool] = None):
        """x (B, T) bytes.  `return_token_logits=None` means `self.training`."""
        if return_token_logits is None:
            return_token_logits = self.training
        h = self.backbone.forward_hidden(x, cutoff=cutoff)
        char_logits = self.head.char_head(h[:, -self.chunk:, :])          # the last `chunk` rows only: the same values
        if return_token_logits:
            return char_logits, self.head.token_head(h)
        return char_logits


_tokenizer_cache = None


def get_gpt2_tokenizer():
    """The GPT-2 BPE tokenizer from the local Hugging Face cache (never from a network), cached; None when
    `transformers` or the files are missing."""
    global _tokenizer_cache
    if _tokenizer_cache is None:
        try:
            from transformers import GPT2TokenizerFast
            _tokenizer_cache = GPT2TokenizerFast.from_pretrained("gpt2", local_files_only=True)
        except Exception:
            return None
    return _tokenizer_cache
