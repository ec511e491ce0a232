"""Compare the gfx950 instructions of the kernels of one .hip file between two
git revisions: which kernels are instruction for instruction the same, which
differ, which are new.  How "the plain kernels stay the code they were" is
checked when a body gains a compile-time form.

    python tools/isa_compare.py <base revision> [file, default csrc/hip/flux.hip] [--fail-on k_a,k_b]

Compiles the file as it is at the base revision and as it is in the working
tree (each against the working tree's headers unless --base-headers), device
code only, with the build's flags, and compares each kernel's body with
comments and local label names removed.  Exit status 1 if a kernel named in
--fail-on differs or is missing.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def kernels(asm):
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s*s_endpgm", asm, re.S | re.M):
        body = re.sub(r";.*", "", m.group(2))
        body = re.sub(r"\.L\w+", "L", body)
        out[m.group(1)] = "\n".join(line.strip() for line in body.splitlines() if line.strip())
    return out


def assembly(src, include_dir):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.s")
        subprocess.run([entry.HIPCC, "-x", "hip", *entry.HIP_FLAGS, "-I", include_dir, "--offload-device-only", "-S",
                        src, "-o", out], check=True)
        return open(out).read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("base")
    ap.add_argument("file", nargs="?", default="cfd-demo2_amd/csrc/hip/flux.hip")
    ap.add_argument("--fail-on", default="")
    a = ap.parse_args()
    inc = os.path.join(ROOT, os.path.dirname(a.file))
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "base_" + os.path.basename(a.file))
        with open(base, "w") as fh:
            fh.write(subprocess.run(["git", "-C", ROOT, "show", f"{a.base}:{a.file}"], check=True, capture_output=True,
                                    text=True).stdout)
        old, new = kernels(assembly(base, inc)), kernels(assembly(os.path.join(ROOT, a.file), inc))
    bad = []
    for k, body in old.items():
        verdict = "missing" if k not in new else "same" if new[k] == body else "DIFFERS"
        print(f"{verdict:8s} {len(body.splitlines()):5d} instructions  {k}")
        if verdict != "same" and any(n and n in k for n in a.fail_on.split(",")):
            bad.append(k)
    for k in new:
        if k not in old:
            print(f"new      {len(new[k].splitlines()):5d} instructions  {k}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
