"""Which kernel instance and grid the launchers of the transform families pick, on the CPU.

tests/launch_trace/launch_trace.hip calls every launcher over the cross product of its selection inputs with
SMX_LAUNCH (csrc/smx_launch.h) recording instead of launching; expected.txt is what the launcher ladders printed before
they became predicates + pick_key (recorded from that code with only its launch statements replaced by the trace
statement, never from the code under test; DESIGN.md section 2 (Kernels) says how to re-record it when an instance is added).
The output must equal it line for line.  One kind of exception: an input that used to fall through a ladder's last
branch onto a neighbouring instance may now be refused, if no caller in smx_api.hip can produce it -- ALLOWED below.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

DIR = os.path.join(ROOT, "tests", "launch_trace")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# (launcher, condition on its inputs -- the columns of its `#` line in expected.txt, guard in smx_api.hip that excludes it)
# The callers' domains the entries lie outside of:
#   fused        nb = Plan::nb (1, 2, 4; 4 on the band-group plan), mode 0 1 2, io 0 1 2, oio -1 or an io value;
#                accumulate only from set_group (band groups: nb 4, f32, dropout stripped); mode 2 only with out NULL
#   fused16, split16_a / _b    nb 1 2 (make_plan: k <= 256 on the sixteen-row plan), mode 0 1 2
#   split_a / split_f / split_b, synth, fused_block    nb = Plan::nb, mode 0 1 2, io 0 1 2
#   full8        mode 0 1 2
#   conv1        io 0 1 2, dir 0 1, nj 8 16 (conv_plan)
#   fs_f         mode 0 ... 4; fs_bgroups only for 5 <= L <= 16
#   fs_big_general    mode 0 ... 4 (through launch_fs_f alone)
# and everywhere: dropout never together with zero-padded rows.
PAD_DROP = "forward_impl / backward_impl: 'fused dropout is not available with zero-padded rows'"
NB = "make_plan sets Plan::nb to 1, 2 or 4 (1 or 2 on the sixteen-row plan); the band-group calls pass 4"
MODE = "the callers pass the literals 0, 1 (forward_impl / backward_impl) and 2 (spectrum_impl)"
GROUPS = "set_group alone sets accumulate: band-group plan, whose calls pass nb = 4 and f32 rows"
ALLOWED = [
    ("fused", "nb == 3", NB),
    ("fused", "mode == 3", MODE),
    ("fused", "acc and out and nb != 4", GROUPS),
    ("fused", "acc and out and mode == 2", "spectrum_impl: the mode-2 launches have out == NULL"),
    ("fused", "acc and out and drop", "post_drop / pre_drop: set_drop(DropCfg{}) when p.groups > 1"),
    ("fused", "pad and drop", PAD_DROP),
    ("fused", "mode == 2 and drop", "spectrum_impl never calls set_drop (decim_args zero-initialises)"),
    ("fused16", "nb in (3, 4)", NB),
    ("fused16", "mode == 3", MODE),
    ("fused16", "pad and drop", PAD_DROP),
    ("split16_a", "nb in (3, 4)", NB),
    ("split16_a", "pad and dflag and drop", PAD_DROP),
    ("split16_b", "nb in (3, 4)", NB),
    ("split16_b", "pad and dflag and drop", PAD_DROP),
    ("split_a", "nb == 3", NB),
    ("split_a", "pad and dflag and drop", PAD_DROP),
    ("split_b", "nb == 3", NB),
    ("split_b", "acc and nb != 4", GROUPS),
    ("split_b", "acc and dflag and drop", "backward_impl: launch_split_b(a, 4, false, s) on the band-group plan"),
    ("split_b", "pad and dflag and drop", PAD_DROP),
    ("split_f", "nb == 3", NB),
    ("split_f", "mode == 3", MODE),
    ("synth", "nb == 3", NB),
    ("full8", "mode == 3", MODE),
    ("fused_block", "nb == 3", NB),
    ("fused_block", "io == 0 and (pad or acc)", "block_forward_impl: layer_shape (rows = n_fft), block_fused_plan (groups == 1)"),
    ("conv1", "io == 3", "io_check at every *_io entry"),
    ("fs_f", "mode == 5", "the callers pass the literals 0 ... 4"),
    ("fs_f", "mode == 1 and fs_bgroups and L <= 32 and not 5 <= L <= 16",
     "backward_impl: bg = (bgo > 0 && fs_grouped_tiles::has(p.L) && ...) ? bgo : 0"),
    ("fs_big_general", "mode == 5", "reached through launch_fs_f alone: modes 0 ... 4"),
]


def _parse(lines):
    """[(launcher, {column: value}, result)] -- columns from the launcher's `# name[, name]: columns` line"""
    cols, out = {}, []
    for ln in lines:
        if ln.startswith("#"):
            names, c = ln[1:].split(":")
            for n in names.split(","):
                cols[n.strip()] = c.split()
            continue
        head, result = ln.split(":", 1)
        name, *vals = head.split()
        assert len(vals) == len(cols[name]), ln
        out.append((name, dict(zip(cols[name], map(int, vals))), result.strip()))
    return out


def _allowed(name, inputs):
    return any(n == name and eval(cond, {}, dict(inputs)) for n, cond, _ in ALLOWED)


@pytest.fixture(scope="module")
def trace():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    subprocess.run(["bash", os.path.join(DIR, "build.sh")], check=True, capture_output=True)
    return subprocess.run([os.path.join(DIR, "launch_trace")], check=True, capture_output=True,
                          text=True).stdout.splitlines()


def test_every_launcher_picks_the_recorded_instance_and_grid(trace):
    expected = open(os.path.join(DIR, "expected.txt")).read().splitlines()
    assert len(trace) == len(expected)
    got, want = _parse(trace), _parse(expected)
    assert len(want) > 5000
    bad = []
    for (n1, i1, r1), (n0, i0, r0) in zip(got, want):
        assert (n1, i1) == (n0, i0)
        if r1 == r0:
            continue
        if r1 == "refused" and not r0.startswith("refused") and _allowed(n0, i0):
            continue
        bad.append(f"{n0} {i0}: recorded '{r0}', now '{r1}'")
    assert not bad, "\n".join(bad[:40])


def test_allow_list_entries_are_all_in_use(trace):
    """an entry that no longer matches a changed line is stale: the list holds nothing it does not need"""
    want = _parse(open(os.path.join(DIR, "expected.txt")).read().splitlines())
    changed = [(n, i) for (n, i, r0), (_, _, r1) in zip(want, _parse(trace)) if r0 != r1]
    for name, cond, _ in ALLOWED:
        assert any(n == name and eval(cond, {}, dict(i)) for n, i in changed), (name, cond)
