#!/usr/bin/env python3
"""Which kernels of a translation unit changed?  Two hipcc objects in, the differing kernel symbols out.

    tools/kdiff.py old/smx_decim.o new/smx_decim.o [--log old.log new.log] [--map 'REGEX=>REPL' ...]

Per kernel symbol of the gfx950 code object: the `llvm-objdump -d` text (addresses and the symbol's own name
removed; the encodings stay, branches are relative) and, with --log, the resource-usage block of a compile log made
with -Rpass-analysis=kernel-resource-usage (one translation unit per log: a parallel build interleaves the lines).
--map rewrites the demangled OLD names before the two sides are paired (renamed templates).  Exit status 1 if
anything differs or is unpaired."""
import argparse, os, re, shutil, subprocess, sys, tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def demangle(names):
    out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout
    return [re.sub(r"^void |\(.*$", "", n.replace("(anonymous namespace)::", "")) for n in out.splitlines()]


def kernels(obj):
    """{mangled name: normalised disassembly} of the kernels (the symbols with a .kd descriptor)"""
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(obj, os.path.join(tmp, "tu.o"))          # (the bundles are written next to the object)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "tu.o"], cwd=tmp, check=True, capture_output=True)
        co = [f for f in os.listdir(tmp) if "gfx950" in f]
        assert len(co) == 1, co
        txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co[0]], cwd=tmp, check=True, capture_output=True,
                             text=True).stdout
        syms = subprocess.run([f"{LLVM}/llvm-objdump", "-t", co[0]], cwd=tmp, check=True, capture_output=True,
                              text=True).stdout
    kd = {l.split()[-1][:-3] for l in syms.splitlines() if l.endswith(".kd")}
    out = {}
    for blk in re.split(r"^[0-9a-f]+ <", txt, flags=re.M)[1:]:
        name, body = blk.split(">:", 1)
        if name in kd:
            body = re.sub(r"(\s|\.\.\.)*$", "", body)        # (objdump's mark for the zero padding behind a section's end)
            out[name] = re.sub(r"// [0-9A-F]+:", "//", body).replace(name, "SELF")
    return out


def resources(log):
    out = {}
    for blk in re.split(r"remark: Function Name: ", open(log).read())[1:]:
        out[blk.split()[0]] = sorted(set(re.findall(r"remark: +([A-Za-z][^:\n]*: \S+)", blk)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old"); ap.add_argument("new")
    ap.add_argument("--log", nargs=2)
    ap.add_argument("--map", action="append", default=[])
    ap.add_argument("--show", type=int, default=0, help="print this many differing lines per kernel")
    a = ap.parse_args()
    sides = []
    for i, obj in enumerate((a.old, a.new)):
        k = kernels(obj)
        res = resources(a.log[i]) if a.log else {}
        names = demangle(list(k))
        if i == 0:
            for m in a.map:
                pat, repl = m.split("=>", 1)
                names = [re.sub(pat, repl, n) for n in names]
        assert len(set(names)) == len(names), "two symbols with one name after --map"
        sides.append({n: (k[s], res.get(s)) for n, s in zip(names, k)})
    old, new = sides
    bad = 0
    for n in sorted(set(old) | set(new)):
        if n not in old or n not in new:
            print(("only in new: " if n in new else "only in old: ") + n); bad += 1
            continue
        what = [w for w, x, y in (("code", old[n][0], new[n][0]), ("resources", old[n][1], new[n][1])) if x != y]
        if what:
            print("differs (" + ", ".join(what) + "): " + n); bad += 1
            d = [f"    - {x}\n    + {y}" for x, y in zip(old[n][0].splitlines(), new[n][0].splitlines()) if x != y]
            print("\n".join(d[:a.show]))
    print(f"{len(old)} kernels in old, {len(new)} in new, {len(set(old) & set(new))} paired, {bad} differing or unpaired"
          + ("" if a.log else " (no resource logs given)"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
