"""Shared by the epoch-end tests (test_eval_cpu.py, test_eval_gpu.py), tests/golden/make_golden_eval.py and
tests/tools/eval_bench.py: seeded corpora, the V02 model loader and the planted-snippet cases of find_snippets.  Nothing
here imports the package under test or the reference."""
import numpy as np
import torch

TILE = 16384                    # positions per tile of the native search (csrc/smx_match.hip); a tile starts where
                                # (address of the position) is a multiple of it modulo the corpus's 16-byte phase
GEOMETRIES = ("conv", "filter")  # V02: seq_len 448 / kernel_len 65 (n_fft = 512) and seq_len 48 / kernel_len 16

WORDS = (b"the", b"cat", b"sat", b"on", b"a", b"mat", b"and", b"then", b"there", b"was", b"once", b"upon", b"time",
         b"little", b"girl", b"who", b"liked", b"to", b"play", b"with", b"her", b"dog", b"in", b"park", b"every", b"day")


def text_corpus(n: int, seed: int) -> bytes:
    """`n` bytes of word-like text: the words above in a seeded order, a full stop and a line feed now and then."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n:
        out += WORDS[int(rng.integers(len(WORDS)))]
        r = int(rng.integers(12))
        out += b".\n" if r == 0 else b", " if r == 1 else b" "
    return bytes(out[:n])


def novel_bytes(n: int, seed: int) -> bytes:
    """`n` printable bytes no word of which is in WORDS: upper-case letters and digits only."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789", dtype=np.uint8)
    return bytes(alphabet[rng.integers(len(alphabet), size=n)].tobytes())


def random_corpus(n: int, seed: int, lo: int = 0, hi: int = 256) -> torch.Tensor:
    """`n` uniform bytes in [lo, hi) on the CPU"""
    return torch.from_numpy(np.random.default_rng(seed).integers(lo, hi, size=n, dtype=np.uint8))


def find_all(corpus: bytes, snips: torch.Tensor) -> torch.Tensor:
    """bytes.find per row of `snips`: the definition the tests hold find_snippets to"""
    return torch.tensor([corpus.find(bytes(row.tolist())) for row in snips.cpu()], dtype=torch.int64)


def planted_case(n: int, L: int, S: int, seed: int, phase: int = 0):
    """(corpus (n,) uint8 with bytes 0..199, snips (S, L) uint8): the corpus is uniform noise; the snippets come in the
    order of `plants` below, as many as S allows, the rest are absent (bytes 200..255).  A present snippet is a slice of the corpus (its
    answer is where bytes.find first sees it, the planted place unless the noise repeats it earlier, which the tests never rely
    on).  `phase`: (address of corpus[0]) mod 16 when the test will view the corpus at that byte offset of an
    allocation -- tile t of the native scan then starts at position t * TILE - phase.
    Planted: at 0; at n - L; straddling every tile boundary by 1, L // 2 and L - 1 bytes; cut off by the end of the
    corpus (present only as a prefix: absent); a duplicate of the first; a twin of the first that shares its first four
    bytes and differs in its last."""
    corpus = random_corpus(n, seed, 0, 200)
    rows = []
    if n >= L:
        places = [0, n - L]
        for edge in range(TILE - phase, n, TILE):
            places += [edge - k for k in (1, L // 2, L - 1) if 0 <= edge - k <= n - L]
        for p in places:
            rows.append(corpus[p:p + L].clone())
        rows.insert(2, rows[0].clone())                              # duplicate
        twin = rows[0].clone()
        twin[-1] = 255 - twin[-1]
        rows.insert(3, twin)                                         # shares the first word (L > 4) and is absent
    cut = torch.cat([corpus[max(0, n - L // 2):], torch.full((L,), 250, dtype=torch.uint8)])[:L]
    rows.insert(min(4, len(rows)), cut)                              # only its prefix is in the corpus, at the very end
    rng = np.random.default_rng(seed + 1)
    while len(rows) < S:
        rows.append(torch.from_numpy(rng.integers(200, 256, size=L, dtype=np.uint8)))
    return corpus, torch.stack(rows[:S])


def load_lm(pkg, z, geom: str, device=None):
    """(model in eval-ready state, cfg, starts) of geometry `geom` from the V02 fixture, through the package `pkg`"""
    cfg = pkg.TrainConfig(d_model=int(z["d_model"]), n_layers=int(z["n_layers"]), seq_len=int(z[geom + ".seq_len"]),
                          kernel_len=int(z[geom + ".kernel_len"]), batch_size=int(z["batch_size"]),
                          val_batches=int(z["val_batches"]), device=str(device or "cpu"))
    model = pkg.FixedSpectralLM(cfg)
    pre = geom + ".sd."
    model.load_state_dict({k[len(pre):]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in z.items()
                           if k.startswith(pre)}, strict=True)
    return model.to(device or "cpu"), cfg, torch.from_numpy(z[geom + ".starts"])
