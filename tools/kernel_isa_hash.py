#!/usr/bin/env python3
"""One line per kernel of csrc/ssx_api.hip: the number of instructions and a SHA-256 of its gfx950 assembly (hipcc -S, no GPU needed) with comments, labels'
numbers and blank lines removed -- two trees whose lines agree for a kernel compile it to the same instructions.  Finer than tools/kernel_resources.py, whose
register counts can stay put while instructions change.
    python tools/kernel_isa_hash.py [-D MACRO ...] [--asm FILE.s]      --asm: hash an assembly file made earlier instead of compiling"""
import hashlib, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernels(text):
    out, cur = {}, None
    for ln in text.split("\n"):
        m = re.match(r"^([A-Za-z_][\w$]*):\s*(;.*)?$", ln)
        if m:
            cur = m.group(1); out[cur] = []; continue
        if ln.startswith(".Lfunc_end"):
            cur = None
        s = re.sub(r";.*", "", ln).strip()
        if cur is None or not s or s.startswith(".") and not s.endswith(":"):
            continue
        out[cur].append(re.sub(r"\.L\w+", "L", s))
    return {k: v for k, v in out.items() if k.startswith("ssx_") and len(v) > 1}


def main():
    args = sys.argv[1:]
    if "--asm" in args:
        text = open(args[args.index("--asm") + 1], errors="replace").read()
    else:
        from simple_spectral_amd import build as _b
        _b.embed_sources()
        with tempfile.TemporaryDirectory() as td:
            asm = os.path.join(td, "k.s")
            subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-S", "--cuda-device-only", "-o", asm,
                                   os.path.join(ROOT, "simple_spectral_amd", "csrc", "ssx_api.hip")] + args, stderr=subprocess.DEVNULL)
            text = open(asm, errors="replace").read()
    print("%-44s %8s  %s" % ("kernel", "lines", "sha256"))
    for k, v in sorted(kernels(text).items()):
        print("%-44s %8d  %s" % (k, len(v), hashlib.sha256("\n".join(v).encode()).hexdigest()[:32]))


if __name__ == "__main__":
    main()
