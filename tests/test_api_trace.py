"""What every C ABI entry does with its arguments -- return code, error text, launches in order -- on the CPU.

tests/api_trace/api_trace.hip links the library's translation units, compiled for the host alone and unchanged, with its
own definitions of the HIP runtime symbols they call, and calls every entry over the plan kinds, call variants, options
and refusals listed there.  expected.txt is what the previous commit's csrc/ printed through the same program (recorded
from the parent, never from the code under test; DESIGN.md section 2 (Kernels) says how to re-record it when an entry
or a plan is added; the "newer ops" section, added together with the move of its entries into smx_api.hip, was recorded
from the previous commit's entries and launchers with only their argument blocks moved into smx_kernels.h).  The output
must equal it line for line: there is no allow list.
"""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

DIR = os.path.join(ROOT, "tests", "api_trace")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# section of expected.txt -> kernels its accepted calls must launch: a sweep that silently misses a plan fails
PLAN_KERNELS = {
    "direct n_fft=1000": ["k_direct_spectrum", "k_direct_filter", "k_direct_synth", "k_gradw", "k_dropout_rows"],
    "direct odd D": ["k_direct_spectrum", "k_direct_synth"],
    "direct k=0": ["k_direct_synth", "memset"],
    "sixteen-row single": ["k_fused16", "k_split16_b", "k_gradw_slab"],
    "sixteen-row split": ["k_split16_a", "k_split_f", "k_split16_b"],
    "single launch, 1 band": ["k_fused<1,", "k_split_b<1,", "k_synth<1"],
    "single launch, 2 bands": ["k_fused<2,", "k_split_b<2,", "k_synth<2"],
    "single launch, 4 bands": ["k_fused<4,", "k_split_b<4,", "k_synth<4"],
    "residue split by shape": ["k_split_a", "k_split_f", "k_split_b", "k_synth"],
    "residue split by option": ["k_split_a", "k_split_f", "k_split_b"],
    "four-step": ["k_fs_a", "k_fs_f", "k_fs_b", "k_fs_synth", "k_dropout_rows"],
    "four-step at 2048 (the pair: eight bands)": ["k_fs_f<8,", "k_full8", "k_synth8"],
    "eight bands": ["k_full8", "k_fused<4,", "k_split_b<4,", "k_synth8", "k_dropout_rows"],
    "band groups, 33 tiles": ["k_fused<4,", "k_edge_partial", "k_edge_synth_acc", "k_edge_slab", "k_split_b<4,",
                              "k_dropout_rows", "k_bx3_synth"],
    "band groups at 2048": ["k_fused<4,", "k_edge_partial", "k_bx3_synth"],
    "force_direct": ["k_bx3_spectrum", "k_bx3_synth"],
    "decim16=0": ["k_bx3_spectrum", "k_bx3_synth"],
    "zero-padded rows": ["k_fused<2,"],
    "four-step, padded rows, Nyquist bin": ["k_fs_a", "k_fs_b"],
    "filter_pack": ["k_pack_w"],
    "row_scale": ["k_fs_gsc"],
    "2-byte rows": ["k_fused<1,", "k_split_a", "k_split_b"],
    "options": ["k_gradw_slab", "k_fs_f_grouped"],      # (fold_gradw = 1, retired: the reduction launch of the default)
    "block entries": ["k_fused_blk", "k_ln_stats", "k_ln_apply", "k_add_rows", "k_ln_bwd", "k_ln_bwd_io", "k_ln_colsum"],
    "convolution": ["k_conv1<", "k_fs_conv<", "k_fs_conv_big", "k_conv_grads"],
    "cfft, phase filter, response": ["k_fs_f<4,3>", "k_fs_big", "k_phase_filter", "k_phase_filter_bwd", "k_conv_response",
                                     "k_conv_response_bwd"],
    "smaller ops": ["k_dwconv3_fwd", "k_dwconv3_bwd", "k_sln_fwd", "k_sln_bwd", "k_pcmul_fwd4", "k_pcmul_bwd4",
                    "k_add_planar", "k_to_planar", "k_gate_fwd", "k_gate_bwd", "k_mix_fwd", "k_mix_bwd", "k_rope_fwd",
                    "k_rope_bwd", "k_res_fwd", "k_res_bwd", "k_ema_fwd", "k_ema_bwd", "k_stream_push", "k_stream_conv",
                    "k_gradw", "k_wfilter", "k_wfilter_gradw", "k_cmul", "k_cmul_gradw", "k_rng_next"],
    "newer ops": ["k_word_targets<1>", "k_word_targets<2>", "k_head_fwd<4,1,1>", "k_head_fwd<1,4,2>", "k_head_bwd<4,1,1>",
                  "k_head_bwd<4,1,2>", "k_ln_colsum", "k_xent_fwd<4,", "k_xent_fwd<1,", "k_xent_fwd_stream", "k_xent_finish",
                  "k_xent_bwd<4,", "k_xent_bwd<1,", "k_xent_bwd_stream", "k_sample_bytes<unsigned char>",
                  "k_sample_bytes<long long>", "k_byte_features<unsigned char,true,512>",
                  "k_byte_features<unsigned char,false,4096>", "k_byte_features<long long,true,4096>",
                  "k_byte_features<long long,false,512>", "k_byte_gb_part", "k_byte_gb_sum", "k_match_scan", "k_match_join",
                  "k_topk_hist", "k_topk_join", "k_topk_pick", "k_topk_count", "k_topk_scan", "k_topk_write",
                  "k_sparse_scatter"],
}
# ... and the refusals that must be on record (by the start of smx_last_error()'s text)
REFUSALS = [
    "workspace is NULL", "workspace has ", "workspace must be 256-byte aligned", "phases must be a combination",
    "io must be SMX_IO_F32", "the band-group plan cannot transform in place", "row_scale is not available on the band-group plan",
    "row_scale is not available on the direct plan", "row_scale is not available on this plan",
    "twiddle tables for N=1536 are not on device", "band-group tables for N=8704 are not on the device",
    "no 2-byte I/O on this plan", "no 2-byte block rows on this plan", "dropout on the eight-band plan needs",
    "dropout with more than 512 bins needs grad_x", "dropout on the direct plan needs grad_x", "xk (saved spectrum) is NULL",
    "SMX_FILTER_PACK_READY without filter_pack", "filter_pack must be 16-byte aligned", "grad_row_scale without row_scale",
    # the newer ops
    "token_bytes must be", "T must be at most 65536", "row_stride must be at least T", "phase and boundary are both NULL",
    "int64 tokens must be 8-byte aligned", "the row head has O = 1 or 2 outputs", "LayerNorm width D=1025 is not supported",
    "grad_h must not alias h or g", "smx_xent_forward: row_stride must be at least V",
    "smx_xent_backward: reduction must be", "grad must not alias logits", "the sampler draws bytes",
    "temperature must be positive and finite, got 0", "top_p is NaN", "n_recent must be in [0, 65536], got 65537",
    "int64 recent ids must be 8-byte aligned", "logits, u, probs must be 4-byte aligned and ids 8-byte aligned",
    "P must be 1 (one row per sequence) or T=", "k must be at most T / 2", "unsupported size (smx_byte_supported)",
    "n_bands must be at least max(1, min(k, W))", "workspace is NULL, 512 bytes required (smx_byte_workspace_bytes)",
    "workspace has 511 bytes, 512 required (smx_byte_workspace_bytes)", "unsupported snippet set (smx_match_supported)",
    "workspace is NULL, 65536 bytes required (smx_match_workspace_bytes)", "first must be 8-byte aligned",
    "max_workgroups must not be negative", "unsupported size (smx_topk_supported)", "k must be in 1..n",
    "smx_topk_select: workspace is NULL", "smx_topk_select: workspace has ", "smx_topk_select: workspace must be 256-byte aligned",
    "smx_topk_compact: workspace is NULL", "smx_topk_compact: workspace must be 256-byte aligned",
    "capacity must not be negative", "m must be in 0..n", "out must be 16-byte aligned",
]
# the code of a misaligned workspace differs by entry (include/smx.h): -1 = SMX_ERR_INVALID, -4 = SMX_ERR_WORKSPACE
MISALIGNED_WS = {"byte_grad_bands": -1, "match_first": -4, "topk_select": -4, "topk_compact": -4}


@pytest.fixture(scope="module")
def trace():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    subprocess.run(["bash", os.path.join(DIR, "build.sh")], check=True, capture_output=True)
    return subprocess.run([os.path.join(DIR, "api_trace")], check=True, capture_output=True, text=True).stdout.splitlines()


def _expected():
    return open(os.path.join(DIR, "expected.txt")).read().splitlines()


def test_every_entry_returns_and_launches_what_was_recorded(trace):
    expected = _expected()
    bad = [f"line {i + 1}: recorded '{w}'\n          now '{g}'" for i, (g, w) in enumerate(zip(trace, expected)) if g != w]
    assert not bad, f"{len(bad)} lines differ (api_trace --verbose prints the arguments behind a digest)\n" + "\n".join(bad[:20])
    assert len(trace) == len(expected)


def test_the_record_reaches_every_plan_kind_and_refusal():
    assert os.path.getsize(os.path.join(DIR, "expected.txt")) < 256 * 1024
    sections, name = {}, None
    for ln in _expected():
        if ln.startswith("## "):
            name = re.sub(r" \[[^\]]*\]$", "", ln[3:])
            sections.setdefault(name, [])
        elif " -> 0: " in ln:
            sections[name].append(ln.split(" -> 0: ", 1)[1])
    for sec, kernels in PLAN_KERNELS.items():
        launched = " | " + " | ".join(sections[sec])
        for k in kernels:
            assert " | " + k in launched, (sec, k)
    refused = [ln.split(" -> ", 1)[1] for ln in _expected() if re.search(r" -> -\d ", ln)]
    for text in REFUSALS:
        assert any(re.match(r"-\d " + re.escape(text), r) for r in refused), text
    for entry, code in MISALIGNED_WS.items():
        lines = [ln for ln in _expected() if ln.startswith(entry + " ") and " ws+128 -> " in ln]
        assert lines and all(re.search(r" ws\+128 -> %d (smx_\w+: )?workspace must be 256-byte aligned$" % code, ln) for ln in lines), entry
    # the plan grid: the default options and the nine single-option changes
    plans = [ln for ln in _expected() if ln.startswith("## plans [")]
    assert len(plans) == 10
