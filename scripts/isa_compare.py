"""Compare the gfx950 disassembly of the trace and reduce kernels between two builds of csrc/kernels.hip (no GPU needed).

    python scripts/isa_compare.py OLD_TREE NEW_TREE

Each tree is a checkout's root (holding simple-raytracer_amd/csrc and include/). kernels.hip is compiled device-only with
the product flags of build.py, the gfx950 code object is unbundled and disassembled with llvm-objdump, and every
srt_trace_kernel instantiation and the plain ordered reduction (srt_reduce_kernel, srt_reduce_kernel<false> since the
denoiser's moments variant made it a template) are compared instruction by instruction, branch offsets and the s_nop
padding between functions left out. Exit status 1 on any difference.
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROCM = Path("/opt/rocm")
REDUCE = {"_Z17srt_reduce_kernel12ReduceParams", "_Z17srt_reduce_kernelILb0EEv12ReduceParams"}


def build(tree, out):
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import build as B
    flags = [f for f in B.FLAGS if not f.startswith("-Rpass")]
    co = out / "kernels.co"
    subprocess.run([B.hipcc(), *flags, "--cuda-device-only", "-c", str(Path(tree) / "simple-raytracer_amd/csrc/kernels.hip"), "-o", str(co)],
                   check=True, capture_output=True)
    elf = out / "kernels.elf"
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
        fs[cur].append(text)
    for body in fs.values():
        while body and body[-1] == "s_nop 0":
            body.pop()
    return fs


def main():
    old_tree, new_tree = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as d:
        a_dir, b_dir = Path(d) / "a", Path(d) / "b"
        a_dir.mkdir()
        b_dir.mkdir()
        a, b = functions(build(old_tree, a_dir)), functions(build(new_tree, b_dir))
    pairs = [(k, k) for k in a if k.startswith("_Z16srt_trace_kernel")]
    pairs += [(ka, kb) for ka in a if ka in REDUCE for kb in b if kb in REDUCE and "ILb1" not in kb]
    bad = 0
    for ka, kb in pairs:
        same = kb in b and a[ka] == b[kb]
        bad += not same
        print(f"{'same' if same else 'DIFFERENT'}  {ka} -> {kb}  ({len(a[ka])} instructions)")
    print(f"{len(pairs)} kernels compared, {bad} different")
    sys.exit(1 if bad or not pairs else 0)


if __name__ == "__main__":
    main()
