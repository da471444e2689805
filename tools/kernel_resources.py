"""Register / scratch budget of the kernels of csrc/*.hip, from the code object's metadata.

    python tools/kernel_resources.py csrc/t2s.hip csrc/t2s_mega.hip > child.txt
    python tools/kernel_resources.py --csrc <other checkout>/gpt-sovits_amd/csrc t2s.hip t2s_mega.hip > parent.txt
    python tools/kernel_resources.py --diff parent.txt child.txt
    python tools/kernel_resources.py --diff parent.txt child.txt --drop-arg t2s_mega_kernel:3 --drop-arg sample_step_kernel:1

Compiles each file for gfx950 (device only, the flags of gsv/build.py) and prints one line per kernel:
demangled name, VGPRs, AGPRs, SGPRs, scratch bytes, spilled VGPRs, spilled SGPRs.  --diff compares two such listings by
name, after dropping template arguments that the second listing added at the end of a name with the value `false` (a
compile-time variant switched off is the kernel the first listing has), and exits 1 if a kernel of the first listing is
missing from the second or has other counts.  --drop-arg KERNEL:N is the other direction: the second listing's KERNEL has lost
template argument N (from 0), so every variant of the first listing is compared with the kernel that is left without it.
Needs no GPU.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed", "-Wno-unused-value"]
FIELDS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count"]


def _tool(name):
    for d in (os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "llvm", "bin"), os.path.dirname(HIPCC), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return name


def resources(src):
    """[(demangled kernel name, [counts in FIELDS order])] of one .hip file"""
    csrc = os.path.dirname(os.path.abspath(src))
    inc = [f"-I{os.path.join(os.path.dirname(os.path.dirname(csrc)), 'include')}", f"-I{csrc}"]   # the checkout's own gsv.h
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "k.co")
        subprocess.run([HIPCC] + FLAGS + inc + ["--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", co], check=True)
        notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = []
    for line in notes.splitlines():
        m = re.match(r"^  (- | {2})(\.[a-z_]+):\s*(\S*)\s*$", line)      # the kernels' own keys: not the nested .args entries
        if not m:
            continue
        if m.group(1) == "- ":
            out.append({})
        out[-1][m.group(2)] = m.group(3).strip("'\"")
    if not out:
        raise SystemExit(f"{src}: no kernel metadata found")
    filt = shutil.which(_tool("llvm-cxxfilt")) or shutil.which("c++filt")
    if not filt:
        raise SystemExit("no demangler found (llvm-cxxfilt or c++filt)")
    names = subprocess.run([filt] + [c[".name"] for c in out], check=True, capture_output=True, text=True).stdout.splitlines()
    return sorted((re.sub(r"^void ", "", n), [int(c.get(f, 0)) for f in FIELDS]) for n, c in zip(names, out))


def _read(path):
    rows = {}
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        name, counts = line.rstrip("\n").rsplit("\t", 1)
        rows[name] = counts
    return rows


def _strip_false(name):
    """k<17, false>(args) -> k<17>(args): a variant parameter that a later commit appended, switched off"""
    head, sep, args = name.partition(">(")
    if head.endswith(", false"):
        return head[:-len(", false")] + sep + args
    return name


def _drop_arg(name, drops):
    """k<17, true>(args) -> k<17>(args) for drops = {"k": 1}: a variant parameter that a later commit removed"""
    head, sep, args = name.partition(">(")
    kernel, lt, targs = head.partition("<")
    n = next((i for k, i in drops.items() if kernel.split("::")[-1] == k), None)
    if n is None or not sep:
        return name
    targs = targs.split(", ")
    return kernel + lt + ", ".join(targs[:n] + targs[n + 1:]) + sep + args


def diff(a, b, drops):
    all_a, pb = _read(a), _read(b)
    twins = {n: _drop_arg(n, drops) for n in all_a if _drop_arg(n, drops) != n}   # first listing's name -> second listing's
    pa = {n: c for n, c in all_a.items() if n not in twins}
    by_name = dict(pb)
    for n, c in pb.items():
        s = _strip_false(n)
        while s != n:
            by_name.setdefault(s, c)
            n, s = s, _strip_false(s)
    bad = 0
    for n, c in sorted(pa.items()):
        if by_name.get(n) != c:
            bad += 1
            print(f"CHANGED  {n}\n    first : {c}\n    second: {by_name.get(n)}")
    for n, t in sorted(twins.items()):     # a variant of the first listing against the one kernel the second has left
        same = pb.get(t) == all_a[n]
        bad += not same
        print(f"{'SAME   ' if same else 'CHANGED'}  {n}\n    first : {all_a[n]}\n    second: {pb.get(t)}  {t.rsplit('>(', 1)[0]}>")
    old = set(pa) | set(twins.values())
    new = [n for n in sorted(pb) if n not in old and _strip_false(n) not in old and _strip_false(_strip_false(n)) not in old]
    print(f"{len(all_a) - bad} of {len(all_a)} kernels of {a} keep their counts in {b}; {len(new)} new kernels")
    for n in new:
        print(f"NEW  {n}\t{pb[n]}")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=os.path.join(ROOT, "gpt-sovits_amd", "csrc"), help="directory the file names are relative to")
    ap.add_argument("--diff", action="store_true", help="compare two listings instead of compiling")
    ap.add_argument("--drop-arg", action="append", default=[], metavar="KERNEL:N",
                    help="with --diff: the second listing's KERNEL has lost template argument N (from 0)")
    ap.add_argument("files", nargs="+")
    a = ap.parse_args()
    if a.diff:
        sys.exit(diff(*a.files, {k: int(n) for k, n in (d.split(":") for d in a.drop_arg)}))
    print("# kernel\t" + " ".join(f.lstrip(".") for f in FIELDS))
    for f in a.files:
        for name, counts in resources(os.path.join(a.csrc, os.path.basename(f))):
            print(f"{name}\t{' '.join(map(str, counts))}")


if __name__ == "__main__":
    main()
