#!/usr/bin/env python3
"""A digest of every kernel's gfx950 assembly, to show that a change left the device code alone (no GPU needed).

    python scripts/kernel_isa_digest.py [--tree ROOT] [--flags="-DSRT_DEV_KNOBS"] [--sources kernels.hip ...] [--out FILE] [--list FILE] [--compare FILE]

Every device translation unit (*.hip) of build.py SOURCES in ROOT (default: this checkout) is compiled with build.py's
FLAGS, the --flags given and `--cuda-device-only -S`. Per kernel (a symbol with a kernel descriptor) the text from its label to
its .Lfunc_end is taken: its instructions and its basic-block labels (where a branch lands is part of the code), with
.LBB<n>_ rewritten to .LBB_ (n is the function's index in its unit, which shifts when neighbours move). Comments, other
labels and every directive are dropped -- data a directive emits inside a function (.long ...) is therefore not hashed; the
kernels here have none. Printed as JSON:

    {kernel (demangled): {"instructions": instruction lines (labels not counted), "sha256": of the normalised text,
                          "amdhsa": the descriptor's lines}}

keyed by the kernel alone, so a kernel that moved to another unit keeps its entry. With --compare, exit status 1 and a
list of the kernels whose entries differ from FILE's (or that only one side has). --list FILE writes the short form, one line
per kernel: the sha256 of its whole entry (instruction count, text digest and descriptor lines), the instruction count, the
name; --compare takes either form.
"""
import argparse
import concurrent.futures
import hashlib
import importlib.util
import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def build_module(tree):
    spec = importlib.util.spec_from_file_location("srt_build_recipe", Path(tree) / "simple-raytracer_amd" / "build.py")
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    return B


def assembly(B, source, flags, out):
    flags = [f for f in B.FLAGS if not f.startswith("-Rpass")] + flags
    r = subprocess.run([B.hipcc(), *flags, "--cuda-device-only", "-S", str(B.CSRC / source), "-o", str(out)], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"hipcc failed on {source}:\n{r.stderr}")
    return out.read_text()


def kernels_of(asm):
    """{mangled kernel: {instructions, sha256, amdhsa}} of one unit's assembly"""
    lines = asm.split("\n")
    desc, cur = {}, None
    for l in lines:
        t = l.split(";")[0].strip()
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", t)
        if m:
            cur = desc.setdefault(m.group(1), [])
        elif t == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and t:
            cur.append(" ".join(t.split()))
    out, name, body = {}, None, []
    for l in lines:
        t = l.split(";")[0].strip()
        m = re.match(r"(\S+):$", t)
        if name is None:
            if m and m.group(1) in desc:
                name, body = m.group(1), []
            continue
        if t.startswith(".Lfunc_end"):
            text = "\n".join(body) + "\n"
            out[name] = {"instructions": sum(not b.endswith(":") for b in body), "sha256": hashlib.sha256(text.encode()).hexdigest(), "amdhsa": desc[name]}
            name = None
        elif t and not m and not t.startswith("."):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(t.split())))
        elif m and m.group(1).startswith(".LBB"):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))  # where a branch lands is part of the code
    return out


def digest(tree, flags, sources=None):
    B = build_module(tree)
    sources = sources or [s for s in B.SOURCES if s.endswith(".hip")]
    res = {}
    with tempfile.TemporaryDirectory() as d, concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:
        for src, asm in zip(sources, pool.map(lambda s: assembly(B, s, flags, Path(d) / (s + ".s")), sources)):
            ks = kernels_of(asm)
            dem = subprocess.run(["c++filt"], input="\n".join(ks), capture_output=True, text=True).stdout.split("\n")
            for mangled, d_name in zip(ks, dem):
                key = d_name.replace("void ", "", 1).replace("(anonymous namespace)::", "").split("(")[0]
                if key in res:
                    raise SystemExit(f"kernel {key} is defined in two units (second: {src})")
                res[key] = ks[mangled]
    return dict(sorted(res.items()))


def listing(res):
    """kernel -> 'entry digest  instructions': the short form of a digest, one line per kernel"""
    return {k: f"{hashlib.sha256(json.dumps(v, sort_keys=True).encode()).hexdigest()} {v['instructions']}" for k, v in res.items()}


def read_digest(path):
    """a digest written with --out (JSON) or with --list, as the short form"""
    txt = Path(path).read_text()
    if txt.lstrip().startswith("{"):
        return listing(json.loads(txt))
    return {l.split(None, 2)[2]: " ".join(l.split(None, 2)[:2]) for l in txt.splitlines() if l.strip()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=str(ROOT), help="checkout to digest (default: this one)")
    ap.add_argument("--flags", default="", help="extra compiler flags, e.g. a variant build's -D switches")
    ap.add_argument("--sources", nargs="*", help="units to compile (default: every *.hip of build.py SOURCES)")
    ap.add_argument("--out", help="write the JSON here instead of printing it")
    ap.add_argument("--list", help="write the short form here: entry digest, instruction count and name per kernel")
    ap.add_argument("--compare", help="a digest written earlier: list the kernels that differ and exit 1 if any does")
    a = ap.parse_args()
    res = digest(a.tree, a.flags.split(), a.sources)
    txt = json.dumps(res, indent=1)
    if a.out:
        Path(a.out).write_text(txt + "\n")
    elif not a.compare and not a.list:
        print(txt)
    if a.list:
        Path(a.list).write_text("".join(f"{v}  {k}\n" for k, v in listing(res).items()))
    if a.compare:
        ref, res = read_digest(a.compare), listing(res)
        bad = [k for k in sorted(ref.keys() | res.keys()) if ref.get(k) != res.get(k)]
        for k in bad:
            print(f"DIFFERENT  {k}" + ("" if k in ref and k in res else f"  only in {'the reference' if k in ref else 'this build'}"))
        print(f"{len(res)} kernels, {len(bad)} different from {a.compare}")
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
