"""Do two trees compile every kernel to the same gfx950 machine code?  (No GPU needed; neither tree is written to.)

    python tools/compare_isa.py <parent tree> [<new tree, default: this one>] [--rename OLD=NEW ...]  > profiles/<log>

Every translation unit of aurora_amd/build.py's SOURCES (the new tree's list and flags, plus what the parent's own list still
names -- the new list alone if the parent's build.py does not load, and the log says so) is compiled in both trees with
COMPILE_FLAGS plus `--cuda-device-only -S`; a unit that only one tree has is reported.  Per kernel (every .amdhsa_kernel symbol)
the instruction text between its label and its .Lfunc_end -- comments and directives dropped, local labels renumbered in order
of appearance -- and the .amdhsa_* descriptor block are compared.  Kernels are matched by demangled name without namespaces
and parameter list, whichever unit they live in; `--rename OLD=NEW` says that the parent's kernel OLD is called NEW in the new
tree.  Exit status 0 iff every kernel of the parent appears exactly once in the new tree with identical text and descriptor,
and the new tree has no kernel besides.
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def build_module(tree: Path):   # the tree's aurora_amd/build.py, loaded without leaving a byte-code cache behind
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location(f"build_{abs(hash(tree))}", tree / "aurora_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernels_of(asm: str) -> dict:
    """name without parameters -> (normalised instruction text, descriptor block)"""
    lines, out = asm.split("\n"), {}
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
        plain = subprocess.run(["c++filt", sym], capture_output=True, text=True, check=True).stdout.strip()
        plain = plain.replace("(anonymous namespace)::", "").replace("aurora::", "").replace("void ", "").split("(")[0]
        assert plain not in out, f"two kernels named {plain} in one unit ({sym}): matching by name would drop one silently"
        out[plain] = ("\n".join(body), desc)
    return out


def compile_tree(tree: Path, units: list, cmd: list, tmp: Path) -> dict:
    """kernel name -> [(unit, text, descriptor), ...] over the tree's device assembly"""
    tmp.mkdir()
    def one(unit):
        dst = tmp / (Path(unit).stem + ".s")
        subprocess.run([*cmd, str(tree / "aurora_amd" / "csrc" / unit), "-o", str(dst)], check=True, stderr=subprocess.DEVNULL)
        return unit, kernels_of(dst.read_text())

    found = defaultdict(list)
    with ThreadPoolExecutor(min(16, len(units))) as pool:
        for unit, ks in pool.map(one, units):
            for name, (text, desc) in ks.items():
                found[name].append((unit, text, desc))
    return found


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent", type=Path)
    ap.add_argument("new", type=Path, nargs="?", default=Path(__file__).resolve().parents[1])
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    trees = {"parent": args.parent.resolve(), "new": args.new.resolve()}
    renames = dict(r.split("=", 1) for r in args.rename)
    build = build_module(trees["new"])
    cmd = [os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc", *build.COMPILE_FLAGS, "--cuda-device-only", "-S"]
    listed = list(build.SOURCES)
    try:
        listed += [u for u in build_module(trees["parent"]).SOURCES if u not in listed]
    except Exception as e:   # (units that only the parent's list names go unseen)
        print(f"# the parent's build.py did not load ({type(e).__name__}: {e}): the new tree's SOURCES alone")
    units = {side: [u for u in listed if (tree / "aurora_amd" / "csrc" / u).exists()] for side, tree in trees.items()}
    print("# " + " ".join(cmd[1:]) + f"  on the {len(units['parent'])} units of the parent tree and the {len(units['new'])} of the new one")
    for u in (u for u in listed if (u in units["parent"]) != (u in units["new"])):
        print(f"# {u}: only in the {'parent' if u in units['parent'] else 'new'} tree")
    with tempfile.TemporaryDirectory() as t:
        parent, new = (compile_tree(trees[side], units[side], cmd, Path(t) / side) for side in ("parent", "new"))
    print(f"\n## {sum(map(len, parent.values()))} kernels in the parent tree, {sum(map(len, new.values()))} in the new one")
    ok, expected = True, set()
    for old, copies in sorted(parent.items(), key=lambda kv: (kv[1][0][0], kv[0])):
        name, label = renames.get(old, old), old if old not in renames else f"{old} = {renames[old]}"
        expected.add(name)
        homes = new.get(name, [])
        if len(copies) != 1 or len(homes) != 1:
            print(f"  {label:60s} parent {[c[0] for c in copies]} -> {[h[0] for h in homes] or 'MISSING'}: not exactly once")
            ok = False
            continue
        (unit, text, desc), (nunit, ntext, ndesc) = copies[0], homes[0]
        same = text == ntext and desc == ndesc
        print(f"  {label:60s} {unit:20s} -> {nunit:20s} {len(text.splitlines()):6d} lines  {'identical' if same else 'DIFFERS'}")
        ok = ok and same
    for name in sorted(set(new) - expected):
        print(f"  {name:60s} only in the new tree: {[h[0] for h in new[name]]}")
        ok = False
    print("\nRESULT: " + ("same machine code" if ok else "MISMATCH"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
