"""Device assembly of translation units of csrc/, this tree against another checkout (the parent commit), kernel for kernel.

    python tools/isa_vs_parent.py PARENT_TREE pauli_stack prnn ... > profiles/<name>_isa_vs_parent.txt

Each unit is compiled for gfx950 to assembly with the flags build.compile_flags gives it in ITS OWN tree.  Every kernel of the parent
is compared instruction for instruction and kernel descriptor for kernel descriptor after removing comments and the per-file function
index in local labels (.LBB<i>_, .Lfunc_end<i>); a kernel is matched by its demangled name, a trailing template argument `false` that
this tree added with a default counting as absent.  Per kernel: lines (descriptor included), VGPRs, SGPRs, LDS and scratch bytes as
the descriptor states them, and the verdict.  Exit status 1 if a kernel of the parent differs or is missing."""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assembly(tree, unit):
    flags = subprocess.run([sys.executable, "-c", "import sys; from rnnwavefunctions_amd import build; "
                            "print('\\n'.join([build.HIPCC] + build.compile_flags(sys.argv[1] + '.hip')))", unit],
                           cwd=tree, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, unit + ".s")
        subprocess.run(flags + ["--cuda-device-only", "-S", os.path.join(tree, "rnnwavefunctions_amd", "csrc", unit + ".hip"), "-o", out],
                       check=True, capture_output=True)
        return open(out).read()


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return [re.sub(r"\(.*$", "", n) for n in out[:len(names)]]


def kernels(text):
    """{demangled name: (normalised lines, resources)} of every kernel (a symbol with a .amdhsa_kernel descriptor)"""
    lines = [re.sub(r"\s*;.*$", "", ln).rstrip() for ln in text.split("\n")]
    lines = [ln for ln in lines if ln.strip()]
    syms = [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel (\S+)", ln))]
    bodies, cur = {s: [] for s in syms}, None
    for ln in lines:
        if ln.endswith(":") and ln[:-1] in bodies:
            cur = ln[:-1]
        elif cur and re.match(r"\.Lfunc_end\d+:", ln):
            cur = None
        if (m := re.match(r"\s*\.amdhsa_kernel (\S+)$", ln)):
            cur = m.group(1)
        if cur:
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            ln = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", ln)
            bodies[cur].append(ln.replace(cur, "SELF"))
        if cur and ln.strip() == ".end_amdhsa_kernel":
            cur = None
    res = {}
    for sym, name in zip(syms, demangle(syms)):
        body = bodies[sym]
        get = lambda key: next((ln.split()[-1] for ln in body if re.match(r"\s*\.amdhsa_" + key + r"\b", ln)), "?")
        res[name] = (body, (get("next_free_vgpr"), get("next_free_sgpr"), get("group_segment_fixed_size"),
                            get("private_segment_fixed_size")))
    return res


def main():
    parent, units = sys.argv[1], sys.argv[2:]
    rows, same, total = [], 0, 0
    for unit in units:
        old, new = kernels(assembly(parent, unit)), kernels(assembly(HERE, unit))
        rows.append("== %s.hip: %d kernels/functions in the parent, %d now" % (unit, len(old), len(new)))
        for name, (body, r) in old.items():
            total += 1
            now = new.get(name) or new.get(re.sub(r">$", ", false>", name))
            verdict = "MISSING" if now is None else "identical" if now[0] == body and now[1] == r else "DIFFERENT"
            same += verdict == "identical"
            rows.append("%-100s %5d lines  vgpr %-4s sgpr %-4s lds %-6s scratch %-4s %s" % ((name, len(body)) + r + (verdict,)))
    print("%s: device assembly with the product flags (build.compile_flags), this change against its parent commit.  %d of the "
          "parent's %d kernels are identical." % (", ".join(u + ".hip" for u in units), same, total))
    print("\n".join(rows))
    return 0 if same == total else 1


if __name__ == "__main__":
    sys.exit(main())
