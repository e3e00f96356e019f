#!/usr/bin/env python3
"""Are the code objects of two builds of the library the same instructions?  For a refactor of
jit_codec.hip: per job, each library (the loader's LONGHAIR_AMD_LIBRARY) precompiles the job's
modules (tools/precompile.py K M BYTES, a child process) into an empty LONGHAIR_AMD_CACHE_DIR of
its own, no GPU; the objects of a job are paired by kernel names and LDS sizes and compared by
`llvm-objdump -d` of the whole object (the instruction text, without the lines that name the
file) and by the per-kernel register, spill and LDS notes (tools/costat.py).  The bytes outside
.text differ with any edit: hipcc names a symbol after a hash of the source text.

For a refactor of kernels.hip (--kernels): the statically compiled kernels of two source trees'
csrc directories, per kernel symbol (compare_static).

Usage: python tools/codiff.py PARENT.so HEAD.so [JOB-NAME-PART ...] > profiles/NAME.txt
       python tools/codiff.py --kernels PARENT/longhair_amd/csrc HEAD/longhair_amd/csrc > profiles/NAME.txt
Exit status 1 if any pair differs."""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

from costat import REPO, kernel_notes
from precompile import KNOB_JOBS

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
NOPLAN = {"LONGHAIR_AMD_NO_FUSED_PLAN": "1"}
PTR = {"LONGHAIR_AMD_PRECOMPILE_PTR": "1"}
FAMILY = {"LONGHAIR_AMD_JIT_DEFINES": "LH_FAMILY=1"}
# (kind, shape, parts, environment)
JOBS = [("strided", s, ("enc", "dec"), {}) for s in
        [(29, 4, 1296), (29, 4, 1304), (29, 8, 1296), (17, 6, 784), (64, 2, 8192), (3, 2, 64), (10, 3, 16384)]]
JOBS += [("nofusedplan", s, ("enc", "dec"), NOPLAN) for s in [(4, 4, 8), (29, 4, 1296)]]
JOBS += [("ptr", s, ("enc", "dec"), PTR) for s in [(29, 4, 1296), (10, 6, 24)]]
JOBS += [("family", s, ("enc",), FAMILY) for s in [(29, 4, 1296), (17, 6, 784)]]
JOBS += [("family", s, ("dec",), FAMILY) for s in [(29, 4, 1296), (17, 4, 784), (4, 5, 96)]]
JOBS += [("knob-" + env["LONGHAIR_AMD_JIT_DEFINES"], s, ("enc", "dec"), env) for s, env in KNOB_JOBS]
JOBS += [("windowed", (3, 13, 2048), ("enc", "dec"), {})]


def objects(lib, shape, part, env, tmp):
    """The job's code objects from `lib`: [(pairing key, file name, sha256, disassembly, notes)]."""
    env = dict(os.environ, LONGHAIR_AMD_LIBRARY=os.path.abspath(lib), LONGHAIR_AMD_CACHE_DIR=tmp,
               LONGHAIR_AMD_PRECOMPILE_PART=part, **env)
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "precompile.py")] + [str(v) for v in shape],
                   env=env, stdout=subprocess.DEVNULL, check=True)
    out = []
    for co in glob.glob(os.path.join(tmp, "**", "*.co"), recursive=True):
        notes = kernel_notes(co)
        text = subprocess.run([OBJDUMP, "-d", co], capture_output=True, text=True, check=True).stdout
        text = "\n".join(ln for ln in text.splitlines() if "file format" not in ln and co not in ln)
        key = sorted((name, f["group_segment_fixed_size"]) for name, f in notes.items())
        out.append((key, os.path.basename(co), hashlib.sha256(open(co, "rb").read()).hexdigest(), text, notes))
    return sorted(out, key=lambda o: o[:2])


def compare(job, libs):
    kind, (k, m, b), part, env = job
    name = f"{kind}-k{k}m{m}b{b}-{part}"
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        pa, he = objects(libs[0], (k, m, b), part, env, ta), objects(libs[1], (k, m, b), part, env, tb)
    rows = []
    if not pa or [o[0] for o in pa] != [o[0] for o in he]:
        return [(name, "-", "-", f"objects do not pair: {[o[0] for o in pa]} against {[o[0] for o in he]}", False)]
    for n, (p, h) in enumerate(zip(pa, he)):
        if p[1] == h[1]:  # the cache names a file by its generated source and options
            verdict, ok = "same cache file name" + ("" if p[2] == h[2] else ", bytes differ"), p[2] == h[2]
        else:
            text, notes = p[3] == h[3], p[4] == h[4]
            verdict = f"`llvm-objdump -d` {'equal' if text else 'DIFFERS'}, notes {'equal' if notes else 'DIFFER'}"
            if not notes:
                verdict += "".join(f"; {kn} {key} {p[4][kn][key]} -> {h[4][kn][key]}" for kn in p[4] for key in p[4][kn]
                                   if p[4][kn][key] != h[4][kn][key])
            ok = text and notes
        rows.append((name + (f"#{n + 1}" if len(pa) > 1 else ""), p[2], h[2], verdict, ok))
    return rows


def static_kernels(csrc, tmp):
    """{kernel: (instructions, notes)} of kernels.hip in `csrc`, compiled for the device alone with
    its Makefile's HIP_FLAGS.  An instruction is its text without address and encoding."""
    make = open(os.path.join(csrc, "Makefile")).read()
    arch, flags = re.findall(r"^ARCH\s*\?=\s*(\S+)$", make, re.M), re.findall(r"^HIP_FLAGS\s*:=\s*(.*[^\\\n])$", make, re.M)
    # one assignment each; the later `HIP_FLAGS +=` lines are the LH_DEBUG and HIP_EXTRA builds' only
    if len(arch) != 1 or len(flags) != 1 or len(re.findall(r"^HIP_FLAGS\s*\+=", make, re.M)) != 2:
        sys.exit(f"codiff: {csrc}/Makefile no longer sets ARCH and HIP_FLAGS the way this mode reads them")
    arch, flags = arch[0], flags[0].replace("$(ARCH)", arch[0]).split()
    fat, co = os.path.join(tmp, "kernels.o"), os.path.join(tmp, "kernels.co")
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", os.path.join(csrc, "kernels.hip"),
                    "-o", fat], check=True)
    subprocess.run([os.path.join(os.path.dirname(OBJDUMP), "clang-offload-bundler"), "--unbundle", "--type=o",
                    "--targets=hipv4-amdgcn-amd-amdhsa--" + arch, "--input=" + fat, "--output=" + co], check=True)
    notes, out, name = kernel_notes(co), {}, None
    for ln in subprocess.run([OBJDUMP, "-d", co], capture_output=True, text=True, check=True).stdout.splitlines():
        sym = re.match(r"[0-9a-f]+ <(\S+)>:", ln)
        if sym:
            name = sym.group(1) if sym.group(1) in notes else None
        elif name and ln.startswith("\t"):
            out.setdefault(name, []).append(ln.split("//")[0].strip())
    return {kn: (out[kn], notes[kn]) for kn in notes}


def compare_static(parent_csrc, head_csrc):
    """One line per kernel of kernels.hip.  A kernel whose argument block kept its layout must be the
    same instructions; one whose kernarg offsets moved (scalar loads and address arithmetic differ)
    must keep its count of instructions that do not begin with s_, and its notes."""
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        with ThreadPoolExecutor(2) as pool:
            pa, he = pool.map(lambda a: static_kernels(*a), [(parent_csrc, ta), (head_csrc, tb)])
    print("# kernel\tinstructions parent -> head\tnot s_* parent -> head\tverdict")
    ok = sorted(pa) == sorted(he)
    for kn in sorted(set(pa) | set(he)):
        if kn not in pa or kn not in he:
            print(f"{kn}\t-\t-\tonly in {'parent' if kn in pa else 'head'}")
            continue
        (pt, pn), (ht, hn) = pa[kn], he[kn]
        vec = [sum(not i.startswith("s_") for i in t) for t in (pt, ht)]
        verdict = "`llvm-objdump -d` equal" if pt == ht else \
            "kernarg layout moved: not s_* count " + ("equal" if vec[0] == vec[1] else "DIFFERS")
        if vec[0] != vec[1]:  # which opcodes
            ops = [Counter(i.split()[0] for i in t if not i.startswith("s_")) for t in (pt, ht)]
            verdict += "".join(f"; {op} {ops[0][op]} -> {ops[1][op]}" for op in sorted(set(ops[0]) | set(ops[1]))
                               if ops[0][op] != ops[1][op])
        verdict += ", notes equal" if pn == hn else ", notes DIFFER" + "".join(
            f"; {key} {pn[key]} -> {hn[key]}" for key in pn if pn[key] != hn[key])
        ok = ok and vec[0] == vec[1] and pn == hn
        print(f"{kn}\t{len(pt)} -> {len(ht)}\t{vec[0]} -> {vec[1]}\t{verdict}")
    sys.exit(0 if ok else 1)


def main():
    if len(sys.argv) < 3 or (sys.argv[1] == "--kernels" and len(sys.argv) != 4):
        sys.exit(__doc__)
    if sys.argv[1] == "--kernels":
        compare_static(*sys.argv[2:4])
    libs, picks = sys.argv[1:3], sys.argv[3:]
    jobs = [(kind, s, part, env) for kind, s, parts, env in JOBS for part in parts]
    jobs = [j for j in jobs if not picks or any(p in f"{j[0]}-k{j[1][0]}m{j[1][1]}b{j[1][2]}-{j[2]}" for p in picks)]
    with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 2))) as pool:
        rows = sorted(r for rs in pool.map(lambda j: compare(j, libs), jobs) for r in rs)
    print("# job\tsha256 parent\tsha256 head\tverdict")
    for r in rows:
        print("\t".join(r[:4]))
    sys.exit(0 if all(r[4] for r in rows) else 1)


if __name__ == "__main__":
    main()
