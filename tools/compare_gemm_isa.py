"""Do two trees compile the GEMM kernels to the same gfx950 machine code?  (No GPU needed.)

    python tools/compare_gemm_isa.py <parent tree> [<new tree, default: this one>]  > profiles/<log>

Both trees' aurora_amd/csrc/gemm*.hip are compiled with build.py's flags plus `--cuda-device-only -S`, once plain and once with
-DA4_EXPERIMENTS (after `tools/gen_gemm_asm.py 1 2 3` in a tree that lacks the variant loops).  Per kernel (every .amdhsa_kernel
symbol) the instruction text between its label and its .Lfunc_end -- comments and directives dropped, local labels renumbered
in order of appearance -- and the .amdhsa_* descriptor block are compared.  Kernels are matched by name without the parameter
list.  Exit status 0 iff
  * every kernel of the parent appears exactly once across the new tree's objects, text and descriptor identical -- except
    linear_kernel_256a4<0> of the plain build, which may differ (it lost the stamp probe's parameter and block);
  * split_f16_kernel is not in gemm_a4's object;
  * in the A4_EXPERIMENTS build linear_kernel_256a4<0..3> are identical too.
"""
import re
import subprocess
import sys
import tempfile
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S"]
HIPCC = "/opt/rocm/bin/hipcc"
CXXFILT = "c++filt"   # (binutils)
LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def kernels_of(asm: str) -> dict:
    """name without parameters -> (normalised instruction text, descriptor block)"""
    lines = asm.split("\n")
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.S | re.M):
        sym, desc = m.group(1), "\n".join(l.strip() for l in m.group(2).split("\n") if l.strip())
        start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        body, names = [], {}
        for l in lines[start + 1:]:
            l = l.split(";")[0].strip()
            if l.startswith(".Lfunc_end"):
                break
            if not l or (l.startswith(".") and not l.endswith(":")):
                continue
            body.append(LABEL.sub(lambda x: names.setdefault(x.group(0), f".L{len(names)}"), l))
        plain = subprocess.run([CXXFILT, sym], capture_output=True, text=True, check=True).stdout.strip()
        plain = plain.replace("(anonymous namespace)::", "").replace("aurora::", "").replace("void ", "").split("(")[0]
        out[plain] = ("\n".join(body), desc)
    return out


def compile_tree(tree: Path, extra: list, tmp: Path) -> dict:
    """translation unit -> kernels_of(its device assembly)"""
    csrc = tree / "aurora_amd" / "csrc"
    if extra and not (csrc / "gemm_a4_loop_v1.inc").exists():
        subprocess.run([sys.executable, str(tree / "tools" / "gen_gemm_asm.py"), "1", "2", "3"], check=True, stdout=subprocess.DEVNULL)
    units = sorted(csrc.glob("gemm*.hip"))

    def one(src):
        dst = tmp / f"{abs(hash((str(tree), tuple(extra))))}_{src.stem}.s"
        subprocess.run([HIPCC, *FLAGS, *extra, str(src), "-o", str(dst)], check=True, stderr=subprocess.DEVNULL)
        return src.name, kernels_of(dst.read_text())

    with ThreadPoolExecutor(4) as pool:
        return dict(pool.map(one, units))


def compare(parent: dict, new: dict, may_differ: set) -> bool:
    where = defaultdict(list)
    for unit, ks in new.items():
        for name in ks:
            where[name].append(unit)
    ok = True
    seen = set()
    for unit, ks in parent.items():
        for name, (text, desc) in sorted(ks.items()):
            if name in seen:
                print(f"  {name:50s} parent {unit}: a second copy of the kernel above")
                continue
            seen.add(name)
            homes = where.get(name, [])
            if len(homes) != 1:
                print(f"  {name:50s} parent {unit} -> {homes or 'MISSING'}: not exactly once")
                ok = False
                continue
            ntext, ndesc = new[homes[0]][name]
            same = text == ntext and desc == ndesc
            verdict = "identical" if same else "differs (allowed: the stamp probe left)" if name in may_differ else "DIFFERS"
            print(f"  {name:50s} parent {unit} -> {homes[0]:15s} {len(text.splitlines()):6d} lines  {verdict}")
            ok = ok and (same or name in may_differ)
    for name in sorted(set(where) - seen):
        print(f"  {name:50s} only in the new tree: {where[name]}")
        ok = False
    return ok


def main() -> int:
    parent = Path(sys.argv[1]).resolve()
    new = Path(sys.argv[2]).resolve() if len(sys.argv) > 2 else Path(__file__).resolve().parents[1]
    print("# hipcc " + " ".join(FLAGS) + "  on aurora_amd/csrc/gemm*.hip of the parent tree and of the new one")
    ok = True
    with tempfile.TemporaryDirectory() as t:
        for title, extra, may_differ in (("default build", [], {"linear_kernel_256a4<0>"}),
                                         ("-DA4_EXPERIMENTS build", ["-DA4_EXPERIMENTS"], set())):
            p, n = compile_tree(parent, extra, Path(t)), compile_tree(new, extra, Path(t))
            print(f"\n## {title}: {sum(len(k) for k in p.values())} kernels in {len(p)} parent objects, "
                  f"{sum(len(k) for k in n.values())} in {len(n)} new objects")
            ok = compare(p, n, may_differ) and ok
            stray = "split_f16_kernel" in n.get("gemm_a4.hip", {})
            print(f"  split_f16_kernel in the new gemm_a4 object: {'YES' if stray else 'no'}"
                  f" (parent: {'yes' if 'split_f16_kernel' in p.get('gemm_a4.hip', {}) else 'no'})")
            ok = ok and not stray
    print("\nRESULT: " + ("same machine code" if ok else "MISMATCH"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
