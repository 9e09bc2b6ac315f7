"""Kernel by kernel comparison of device assembly across files: does every kernel of the NEW files have the instruction
stream, the .amdhsa_ descriptor and the metadata values it has in the OLD files?  For moves of kernels between translation
units, where a whole-file diff is useless (the index in a basic-block label follows the kernel's position in its file).

Emit the assembly with the Makefile's flags for each file and --cuda-device-only -S, then
usage: python scripts/prof/kernel_asm_diff.py OLD.s[,OLD2.s...] NEW.s [NEW2.s ...]
Per kernel: assembler comments (from ';') are stripped, the function index in .LBB<n>_ / .LJTI<n>_ / .Ltmp<n> / .Lfunc_*<n>
labels is erased, __hip_cuid_ lines are dropped.  Prints one line per NEW file (kernels compared, kernels identical), every
difference, and the kernels of OLD that no NEW file holds; exit status 1 if anything differs or is missing."""
import re
import subprocess
import sys

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size")


def _norm(lines):
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip() or "__hip_cuid_" in ln:
            continue
        ln = re.sub(r"\.(LBB|LJTI|Ltmp)\d+", r".\1", ln)
        ln = re.sub(r"\.Lfunc_(\w+?)\d+", r".Lfunc_\1", ln)
        out.append(ln)
    return out


def kernels(path):
    """{mangled name: (instruction lines, descriptor lines, {metadata key: value})} of one assembly file."""
    text = open(path).read().split("\n")
    desc, i = {}, 0
    while i < len(text):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", text[i])
        if m:
            j = i
            while ".end_amdhsa_kernel" not in text[j]:
                j += 1
            desc[m.group(1)] = _norm(text[i + 1:j])
            i = j
        i += 1
    body = {}
    for i, ln in enumerate(text):
        m = re.match(r"(\S+):\s*(;.*)?$", ln)
        if m and m.group(1) in desc and m.group(1) not in body:
            j = i
            while not re.match(r"\.Lfunc_end\d+:", text[j]):
                j += 1
            body[m.group(1)] = _norm(text[i + 1:j])
    meta = {}
    start = next(i for i, ln in enumerate(text) if ln.startswith("amdhsa.kernels:"))
    entry = None
    for ln in text[start + 1:]:
        if re.match(r"  - \.", ln):
            entry = {}
        elif not ln.startswith("    "):
            if ln.startswith("amdhsa.") or ln.startswith("..."):
                break
        m = re.match(r"\s+(?:- )?(\.[a-z_]+):\s+(\S+)$", ln)
        if m and entry is not None:
            if m.group(1) == ".name":
                meta[m.group(2)] = entry
            if m.group(1) in META:
                entry[m.group(1)] = m.group(2)
    assert set(desc) == set(body) == set(meta), (path, len(desc), len(body), len(meta))
    return {k: (body[k], desc[k], meta[k]) for k in desc}


def main(argv):
    old = {}
    for p in argv[0].split(","):
        old.update(kernels(p))
    seen, bad = set(), 0
    for p in argv[1:]:
        new = kernels(p)
        same = 0
        for name, (b, d, m) in sorted(new.items()):
            assert name not in seen, f"{name} in two new files"
            seen.add(name)
            if name not in old:
                print(f"  NOT IN OLD: {name}")
                continue
            ob, od, om = old[name]
            what = [w for w, x, y in (("instructions", ob, b), ("descriptor", od, d), ("metadata", om, m)) if x != y]
            if what:
                print(f"  DIFFERS ({', '.join(what)}; instruction lines {len(ob)} / {len(b)}): {name}")
                for k in META:
                    if om.get(k) != m.get(k):
                        print(f"    {k}: {om.get(k)} / {m.get(k)}")
            else:
                same += 1
        bad += len(new) - same
        print(f"{p}: {len(new)} kernels compared, {same} identical")
    missing = sorted(set(old) - seen)
    for name in missing:
        print(f"  MISSING FROM NEW: {name}")
    print(f"old: {len(old)} kernels, new: {len(seen)}; {len(seen & set(old)) - bad if not missing else '?'} identical")
    return 1 if bad or missing else 0


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    if sys.argv[1] == "--demangle":           # names of a file's kernels, demangled (for the kernel -> file map)
        names = "\n".join(kernels(sys.argv[2]))
        print(subprocess.run(["c++filt"], input=names, capture_output=True, text=True).stdout, end="")
        sys.exit(0)
    sys.exit(main(sys.argv[1:]))
