#!/usr/bin/env python3
"""Device code of this tree's csrc units against a commit's, kernel by kernel.  CPU only: it compiles, it runs nothing.

    python tools/compare_kernel_code.py REV [--units mdx_pairs,mdx_sw] [--jobs 8]

`git archive REV` goes into a temporary directory; every csrc/*.hip of both trees is compiled for the device with the
Makefile's CXXFLAGS plus --save-temps -Rpass-analysis=kernel-resource-usage; the device assembly is cut per function (a kernel:
from its label to .end_amdhsa_kernel, so the kernel descriptor is compared too; a device function the inliner kept: to its end
label), names demangled, comments dropped, and normalised as in profiles/r09_unit_split.md: the numbers of .LBB<n>_ / .Lfunc_* /
.Ltmp labels and the `mdx::` / `(anonymous namespace)::` components of names.  Per unit it prints what is identical, different,
new or gone, with the compiler's resource remarks beside what is not identical.  A function that is gone from one unit and new
under the same name in another is compared across the two and printed, where it left, as "moved, identical" or "moved,
different".  Exit status 1 when anything differs, is new or is gone (a move that left the code identical is none of these).
"""
import argparse
import concurrent.futures
import difflib
import pathlib
import re
import subprocess
import sys
import tempfile

REPO = pathlib.Path(__file__).resolve().parents[1]
PACKAGE = "diffusion_for_multi_scale_molecular_dynamics_amd"
REMARKS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
           "LDS Size [bytes/block]")


def makefile_flags(csrc: pathlib.Path):
    """(hipcc, CXXFLAGS) as csrc/Makefile sets them, $(ARCH) filled in."""
    text = (csrc / "Makefile").read_text().replace("\\\n", " ")
    value = {name: re.search(rf"^{name}\s*\??=\s*(.*)$", text, re.M).group(1).strip() for name in ("HIPCC", "ARCH", "CXXFLAGS")}
    return value["HIPCC"], value["CXXFLAGS"].replace("$(ARCH)", value["ARCH"]).split()


def compile_unit(source: pathlib.Path, out: pathlib.Path):
    """Device assembly and resource remarks of one unit, compiled in a directory of its own (--save-temps writes there)."""
    out.mkdir(parents=True)
    hipcc, flags = makefile_flags(source.parent)
    run = subprocess.run([hipcc, *flags, "--cuda-device-only", "--save-temps", "-Rpass-analysis=kernel-resource-usage", "-c",
                          "-o", "unit.o", str(source)], cwd=out, capture_output=True, text=True)
    if run.returncode != 0:
        raise RuntimeError(f"{source}: hipcc failed\n{run.stderr[-4000:]}")
    assembly, = out.glob("*-amdgcn-amd-amdhsa-*.s")
    return functions_of(assembly.read_text()), remarks_of(demangle(run.stderr))


def demangle(text: str) -> str:
    return subprocess.run(["c++filt"], input=text, capture_output=True, text=True, check=True).stdout


def normalise(line: str) -> str:
    line = line.split(";", 1)[0].rstrip()
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    line = re.sub(r"\.(Lfunc_begin|Lfunc_end|Ltmp)\d+", r".\1", line)
    return line.replace("mdx::", "").replace("(anonymous namespace)::", "")


def functions_of(assembly: str):
    """{normalised name: normalised lines} of every function of the device assembly."""
    lines = assembly.splitlines()
    kernels = {m.group(1) for line in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line))}
    typed = {m.group(1) for line in lines if (m := re.match(r"\s*\.type\s+(\S+),@function", line))}
    cut, name = [], None                       # cut on the mangled names, demangled in one pass afterwards
    for line in lines:
        if name is None:
            if (m := re.match(r"([\w.$]+):", line)) and m.group(1) in typed | kernels:
                name = m.group(1)
                cut.append("@@function " + name)
            continue
        cut.append(line)
        if ".end_amdhsa_kernel" in line if name in kernels else re.match(r"\s*\.Lfunc_end\d+:", line):
            name = None
    found, body = {}, None
    for line in demangle("\n".join(cut)).splitlines():
        if line.startswith("@@function "):
            body = found.setdefault(normalise(line[len("@@function "):]), [])
        elif (text := normalise(line)).strip():
            body.append(text)
    return found


def remarks_of(stderr: str):
    """{normalised function name: 'SGPRs 20 VGPRs 12 ...'} from the kernel-resource-usage remarks."""
    found, name = {}, None
    for line in stderr.splitlines():
        if m := re.search(r"Function Name: (.*?) \[-Rpass", line):
            name = normalise(m.group(1))
            found[name] = {}
        elif name and (m := re.search(r":\s+([A-Za-z][^:]*?): (\S+) \[-Rpass", line)) and m.group(1) in REMARKS:
            found[name][m.group(1)] = m.group(2)
    return {name: " ".join(f"{key.split(' [')[0]} {values.get(key, '?')}" for key in REMARKS) for name, values in found.items()}


def instructions(body) -> int:
    return sum(1 for line in body if re.match(r"\s+[a-z]", line))


def compared(name, args, old_body, new_body, old_remarks, new_remarks) -> str:
    """The report of a function present on both sides: instruction counts, remarks, and --diff lines of the difference."""
    return (f"{name}\n        instructions {instructions(old_body)} -> {instructions(new_body)}\n"
            f"        {args.rev}: {old_remarks.get(name, 'no remark')}\n        tree: {new_remarks.get(name, 'no remark')}"
            + "".join("\n        | " + line for line in list(difflib.unified_diff(old_body, new_body, args.rev, "tree", n=2,
                                                                                  lineterm=""))[:args.diff]))


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("rev")
    parser.add_argument("--units", default="", help="comma-separated unit names without .hip (default: every unit)")
    parser.add_argument("--jobs", type=int, default=8, help="compilations side by side (at most 16)")
    parser.add_argument("--identical", action="store_true", help="list the identical functions too, with their resource remarks")
    parser.add_argument("--diff", type=int, default=0, metavar="LINES", help="print this much of the diff of each different function")
    args = parser.parse_args()
    wanted = {u for u in args.units.split(",") if u}
    with tempfile.TemporaryDirectory(prefix="compare_kernel_code_") as scratch:
        scratch = pathlib.Path(scratch)
        (scratch / "rev").mkdir()
        archive = subprocess.run(["git", "-C", str(REPO), "archive", args.rev], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", str(scratch / "rev")], input=archive, check=True)
        trees = {"rev": scratch / "rev" / PACKAGE / "csrc", "tree": REPO / PACKAGE / "csrc"}
        units = sorted({p.stem for csrc in trees.values() for p in csrc.glob("*.hip")} & wanted if wanted else
                       {p.stem for csrc in trees.values() for p in csrc.glob("*.hip")})
        with concurrent.futures.ThreadPoolExecutor(max(1, min(args.jobs, 16))) as pool:
            built = {(side, unit): pool.submit(compile_unit, csrc / f"{unit}.hip", scratch / "out" / side / unit)
                     for side, csrc in trees.items() for unit in units if (csrc / f"{unit}.hip").exists()}
            built = {key: job.result() for key, job in built.items()}
    kinds = ("identical", "different", "moved, identical", "moved, different", "new", "gone")
    report = {unit: {kind: {} for kind in kinds} for unit in units}          # unit -> kind -> {function name: text}
    for unit in units:
        old_code, old_remarks = built.get(("rev", unit), ({}, {}))
        new_code, new_remarks = built.get(("tree", unit), ({}, {}))
        rows = report[unit]
        for name in sorted(old_code.keys() | new_code.keys()):
            if name not in new_code:
                rows["gone"][name] = f"{name}\n        {args.rev}: {old_remarks.get(name, 'no remark')}"
            elif name not in old_code:
                rows["new"][name] = f"{name}\n        tree: {new_remarks.get(name, 'no remark')}"
            elif old_code[name] != new_code[name] or old_remarks.get(name) != new_remarks.get(name):
                rows["different"][name] = compared(name, args, old_code[name], new_code[name], old_remarks, new_remarks)
            else:
                rows["identical"][name] = f"{name}\n        {new_remarks.get(name, 'no remark')}"
    # a function gone from one unit and new under the same name in another has moved: the pair is compared like any other and
    # reported where it left (a second unit that lost the same function, a dead copy, keeps its "gone")
    for unit in units:
        for name in list(report[unit]["gone"]):
            if to := next((other for other in units if name in report[other]["new"]), None):
                (old_code, old_remarks), (new_code, new_remarks) = built[("rev", unit)], built[("tree", to)]
                same = old_code[name] == new_code[name] and old_remarks.get(name) == new_remarks.get(name)
                del report[unit]["gone"][name], report[to]["new"][name]
                report[unit]["moved, identical" if same else "moved, different"][name] = f"{unit}.hip -> {to}.hip: " + compared(
                    name, args, old_code[name], new_code[name], old_remarks, new_remarks)
    for unit in units:
        rows = report[unit]
        print(f"{unit}.hip: " + ", ".join(f"{len(rows[kind])} {kind}" for kind in kinds if rows[kind] or "moved" not in kind))
        for kind in kinds[1:] + (kinds[:1] if args.identical else ()):
            for row in rows[kind].values():
                print(f"    {kind}: {row}")
    total = {kind: sum(len(report[unit][kind]) for unit in units) for kind in kinds}
    print("all units: " + ", ".join(f"{count} {kind}" for kind, count in total.items()))
    return 1 if total["different"] or total["moved, different"] or total["new"] or total["gone"] else 0

if __name__ == "__main__":
    sys.exit(main())
