"""Compare the gfx950 disassembly of every device function between two builds of csrc/ (no GPU needed).

    python scripts/isa_compare.py OLD_TREE NEW_TREE

Each tree is a checkout's root (holding simple-raytracer_amd/csrc and include/). Every source of build.py SOURCES is
compiled device-only with the product flags of build.py, its gfx950 code object is unbundled and disassembled with
llvm-objdump, and every function in it is compared instruction by instruction, branch offsets, the s_nop padding
between functions and the pc-relative literal that follows an s_getpc_b64 (the distance to a constant table of the same object,
which moves when another function is added to the source) left out. A function that only one side has counts as a difference; the plain ordered reduction is
matched across its rename to srt_reduce_kernel<false> (a template since the denoiser's moments variant), and the twelve temporal
set-ups across theirs to srt_temporal_kernel<MOTION, ILLUM, CLAMP>. A function that differs prints both counts. Exit status 1 on
any difference; with --allow-new, functions that only the new tree has do not count.
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROCM = Path("/opt/rocm")
RENAMED = {"_Z17srt_reduce_kernel12ReduceParams": "_Z17srt_reduce_kernelILb0EEv12ReduceParams"}  # old name -> new name
TEMPORAL_SETUP = re.compile(r"^_ZN12_GLOBAL__N_1\d+srt_temporal_(setup|motion|deform)(_illum)?(_clamp)?_kernelENS_14TemporalParamsE")


def renamed(name):
    """an old tree's function under the name the new tree gives it: the table above, and a scene-class kernel from before the
    plane form was a template parameter is the class's own kernel, plane form 0"""
    name = RENAMED.get(name, name)
    m = TEMPORAL_SETUP.match(name)
    if m:  # the twelve temporal set-ups from before they were srt_temporal_kernel<MOTION, ILLUM, CLAMP>
        motion = {"setup": 0, "motion": 1, "deform": 2}[m.group(1)]
        return f"_ZN12_GLOBAL__N_119srt_temporal_kernelILi{motion}ELb{int(bool(m.group(2)))}ELb{int(bool(m.group(3)))}EEEvNS_9SetupArgsIXT_EXT1_EEE"
    return re.sub(r"^(_Z22srt_trace_scene_kernelILj\d+ELb[01])(EEv11TraceParams)$", r"\1ELj0\2", name)


def build_module():
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import build as B
    return B


def build(B, tree, source, out):
    flags = [f for f in B.FLAGS if not f.startswith("-Rpass")]
    co = out / f"{source}.co"
    subprocess.run([B.hipcc(), *flags, "--cuda-device-only", "-c", str(Path(tree) / "simple-raytracer_amd/csrc" / source), "-o", str(co)],
                   check=True, capture_output=True)
    elf = out / f"{source}.elf"
    subprocess.run([str(ROCM / "llvm/bin/clang-offload-bundler"), "--unbundle", "--type=o", f"--input={co}",
                    f"--targets=hipv4-amdgcn-amd-amdhsa--{B.ARCH}", f"--output={elf}"], check=True)
    return elf


def functions(elf):
    out = subprocess.run([str(ROCM / "llvm/bin/llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", str(elf)],
                         capture_output=True, text=True, check=True).stdout
    fs, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^([0-9a-f]+ )?<(.+)>:$", line)
        if m:
            cur = m.group(2)
            fs[cur] = []
            continue
        text = re.sub(r"//.*", "", line).strip()
        if cur is None or not text or text == "...":
            continue
        if text.startswith(("s_branch", "s_cbranch")):
            text = text.split()[0]
        if text.startswith("s_add_u32") and fs[cur] and fs[cur][-1].startswith("s_getpc_b64"):
            text = text.rsplit(",", 1)[0]  # pc + literal: where the object's constants lie from here
        fs[cur].append(text)
    for body in fs.values():
        while body and body[-1] == "s_nop 0":
            body.pop()
    return fs


def main():
    allow_new = "--allow-new" in sys.argv
    old_tree, new_tree = [x for x in sys.argv[1:] if x != "--allow-new"][:2]
    B = build_module()
    a, b = {}, {}
    with tempfile.TemporaryDirectory() as d:
        a_dir, b_dir = Path(d) / "a", Path(d) / "b"
        a_dir.mkdir()
        b_dir.mkdir()
        for src in B.SOURCES:  # (a source only one tree has: its functions are reported as "only in")
            if (Path(old_tree) / "simple-raytracer_amd/csrc" / src).exists():
                a.update({(src, renamed(k)): v for k, v in functions(build(B, old_tree, src, a_dir)).items()})
            if (Path(new_tree) / "simple-raytracer_amd/csrc" / src).exists():
                b.update({(src, k): v for k, v in functions(build(B, new_tree, src, b_dir)).items()})
    names = sorted(a.keys() | b.keys())
    bad = 0
    for k in names:
        same = k in a and k in b and a[k] == b[k]
        bad += not same and not (allow_new and k not in a)
        where = "" if k in a and k in b else f"  only in {'old' if k in a else 'new'}"
        word = "same" if same else "new" if allow_new and k not in a else "DIFFERENT"
        count = f"{len(a[k])} -> {len(b[k])}" if k in a and k in b and not same else len(a.get(k, b.get(k)))
        print(f"{word}  {k[0]}  {k[1]}  ({count} instructions){where}")
    print(f"{len(names)} functions of {len(B.SOURCES)} sources compared, {bad} different")
    sys.exit(1 if bad or not names else 0)


if __name__ == "__main__":
    main()
