#!/usr/bin/env python3
"""Machine-code identity of compilation units between two trees: a refactor that must not change a kernel proves it here.

    python profiles/compare_kernel_isa.py OLD_TREE NEW_TREE > profiles/preprocess_split_isa.txt      # CPU only: hipcc -S cross-compiles gfx950
    python profiles/compare_kernel_isa.py OLD_TREE NEW_TREE mlp hexplane binning > profiles/switches_retired_isa.txt
    python profiles/compare_kernel_isa.py OLD_TREE NEW_TREE binning=binning+radix_sort knn --rename 'k_sorted_counts<false>=k_sorted_counts' \
        --removed 'k_sorted_counts<true>' ... > profiles/radix_sort_split_isa.txt

OLD_TREE is a checkout of the commit before the change (`git worktree add` / `git archive`), NEW_TREE a checkout at or after it.  Every further
argument names a unit of emd_amd/csrc (`mlp`: the old mlp.hip against the new one) or a split `OLD=NEW1+NEW2`; with none it is
`preprocess=preprocess+standalone_ops`, the split of the projection unit.  The units are compiled to assembly the way profiles/make_isa_mix.py
does (hipcc -S --cuda-device-only), both sides with the flags NEW_TREE's Makefile gives for the new unit (`make print-flags-<unit>`; the two
halves of the preprocess split both carry -ffp-contract=off -fno-slp-vectorize, as preprocess.hip did before).  For every `.amdhsa_kernel`
symbol the instruction text of the function and its `.amdhsa_*` descriptor block are compared after exactly these normalisations:

    * the function index inside local labels (.LBB<n>_<m> -> .LBB_<m>, .Lfunc_begin<n> / .Lfunc_end<n> likewise): a kernel's position in its unit;
    * the __hip_cuid_* symbol (a hash of the compilation);
    * .file / .loc / .ident lines, comments and blank lines.

A kernel whose symbol changes (a template parameter dropped) is paired with its successor by `--rename 'OLD=NEW'`, one per kernel, and a kernel
that is dropped on purpose is named by `--removed 'OLD'`; both take the name as the table prints it or the mangled symbol, every pairing and
removal is printed, none is guessed, and one that matches nothing fails the run.  A renamed kernel that lost arguments has a smaller argument
segment: for a renamed kernel, and for no other, a difference in the `.amdhsa_kernarg_size` line alone is printed as it is and does not fail the run.

Passes (exit status 0) when, for every argument, the kernel symbols of the new units together are exactly those of the old unit (after the renames,
less the removed ones), no symbol is in two of them (nor, unless it has internal linkage, in the units of two arguments), and every kernel is
identical.  One line per kernel: name, VGPRs, SGPRs, LDS bytes, scratch bytes, verdict."""
import difflib
import os
import re
import subprocess
import sys
import tempfile
import textwrap

DEFAULT_UNITS = ("preprocess=preprocess+standalone_ops",)


def unit_flags(tree, unit):
    csrc = os.path.join(tree, "emd_amd", "csrc")
    out = subprocess.run(["make", "-s", "--no-print-directory", "-C", csrc, f"print-flags-{unit}"], check=True, capture_output=True, text=True).stdout
    return [f for f in out.split() if not f.startswith("-I")]


def assemble(tree, unit, flags):
    csrc = os.path.join(tree, "emd_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, unit + ".s")
        cmd = ["/opt/rocm/bin/hipcc", *flags, f"-I{os.path.join(tree, 'include')}", "-S", "--cuda-device-only", os.path.join(csrc, unit + ".hip"), "-o", out]
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, cwd=csrc)
        if r.returncode:
            sys.exit(f"{' '.join(cmd)}\n{r.stderr}")
        return open(out).read().splitlines()


def normalise(lines):
    out = []
    for l in lines:
        s = l.split(";")[0].strip()
        if not s or s.startswith((".file", ".loc", ".ident")):
            continue
        s = re.sub(r"\.(LBB|Lfunc_begin|Lfunc_end)\d+", r".\1", s)
        s = re.sub(r"__hip_cuid_\w+", "__hip_cuid", s)
        out.append(" ".join(s.split()))
    return out


def kernels_of(lines):
    """-> {symbol: dict(body, desc, vgpr, sgpr, lds, scratch)}"""
    res = {}
    for k, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if not m:
            continue
        sym = m.group(1)
        end = next(j for j in range(k, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        desc = lines[k + 1:end]
        start = next(j for j, x in enumerate(lines) if x.startswith(sym + ":"))
        fend = next(j for j in range(start, len(lines)) if lines[j].startswith(".Lfunc_end"))
        # the register / memory figures the compiler prints behind the function
        info = {}
        for j in range(fend, min(fend + 40, len(lines))):
            mm = re.match(r";\s*(TotalNumSgprs|TotalNumVgprs|ScratchSize|LDSByteSize):\s*(\d+)", lines[j])
            if mm:
                info[mm.group(1)] = int(mm.group(2))
        res[sym] = dict(body=normalise(lines[start + 1:fend]), desc=normalise(desc), vgpr=info["TotalNumVgprs"], sgpr=info["TotalNumSgprs"],
                        lds=info["LDSByteSize"], scratch=info["ScratchSize"])
    return res


def demangle(syms):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(syms), check=True, capture_output=True, text=True).stdout.split("\n")
        return {s: re.sub(r"^void |\(anonymous namespace\)::|\(.*", "", d) for s, d in zip(syms, out)}
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in syms}


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    old_tree, new_tree = (os.path.abspath(p) for p in sys.argv[1:3])
    # --rename 'OLD=NEW' / --removed 'OLD': explicit pairings of the symbols that change
    rest, renames, removed = [], {}, set()
    it = iter(sys.argv[3:])
    for a in it:
        if a == "--rename":
            o, n = next(it).split("=")
            renames[o.strip()] = n.strip()
        elif a == "--removed":
            removed.add(next(it).strip())
        else:
            rest.append(a)
    unused = set(renames) | removed
    # [(old unit, new units)]
    groups = [(a.split("=")[0], tuple(a.split("=")[-1].split("+"))) for a in (rest or DEFAULT_UNITS)]
    new_units = [u for _, us in groups for u in us]
    flags = {u: unit_flags(new_tree, u) for u in new_units}
    hips = lambda units: " / ".join(u + ".hip" for u in units)
    flag_sets = sorted({" ".join(f) for f in flags.values()})
    flag_text = flag_sets[0] if len(flag_sets) == 1 else "; ".join(f"{u}.hip: {' '.join(flags[u])}" for u in new_units)
    print(textwrap.fill(f"profiles/compare_kernel_isa.py: every kernel of the old emd_amd/csrc/{hips(o for o, _ in groups)} against the same kernel of the new "
                        f"{hips(new_units)}; `hipcc -S --cuda-device-only`, gfx950, flags:", 150, initial_indent="# ", subsequent_indent="# ") + " " + flag_text)
    print("# compared: the instruction text of the function and its .amdhsa_* descriptor, modulo local-label function indices, __hip_cuid_*, comments")
    print(f"# {'kernel':28s} {'unit':15s} {'VGPRs':>5s} {'SGPRs':>5s} {'LDS B':>6s} {'scratch B':>9s}  verdict")
    ok = True
    n_removed = [0, 0]                     # kernels removed on purpose, renamed kernels identical but for the kernarg size
    n_old, n_new, seen = {}, {}, {}          # seen: symbol -> new unit over ALL arguments (anonymous-namespace symbols are per unit: kept per argument only)
    for old_unit, units in groups:
        old, new, where = kernels_of(assemble(old_tree, old_unit, flags[units[0]])), {}, {}
        for u in units:
            ks = kernels_of(assemble(new_tree, u, flags[u]))
            for s in ks:
                if s in where or s in seen:
                    print(f"# FAIL: {s} is in {where.get(s) or seen[s]}.hip and in {u}.hip")
                    ok = False
                where[s] = u
                if "_GLOBAL__N_" not in s:
                    seen[s] = u
            new.update(ks)
            n_new[u] = len(ks)
        n_old[old_unit] = len(old)
        names = demangle(sorted(set(old) | set(new)))
        named = lambda syms, x: [s for s in syms if x in (s, names[s])]
        note = {}                                # new symbol -> the old name it was paired with
        for o_name, n_name in renames.items():
            os_, ns_ = named(old, o_name), named([s for s in new if s not in old], n_name)
            if not os_:
                continue                         # (a kernel of another argument's unit)
            unused.discard(o_name)
            if len(os_) != 1 or len(ns_) != 1:
                print(f"# FAIL: --rename {o_name}={n_name}: {len(os_)} old and {len(ns_)} new kernels of these names in {old_unit}.hip -> {hips(units)}")
                ok = False
                continue
            print(f"# --rename: {names[os_[0]]} ({os_[0]}) -> {names[ns_[0]]} ({ns_[0]})")
            k = old.pop(os_[0])
            old[ns_[0]] = dict(k, body=[l.replace(os_[0], ns_[0]) for l in k["body"]], desc=[l.replace(os_[0], ns_[0]) for l in k["desc"]])
            note[ns_[0]] = names[os_[0]]
        for o_name in sorted(removed):
            for s in named(old, o_name):
                if s in new:
                    continue
                unused.discard(o_name)
                k = old.pop(s)
                n_old[old_unit] -= 1
                n_removed[0] += 1
                print(f"{names[s]:30s} {'-':15s} {k['vgpr']:5d} {k['sgpr']:5d} {k['lds']:6d} {k['scratch']:9d}  removed (--removed: in the old unit only)  ({s})")
        for s in sorted(set(old) | set(new), key=lambda s: (where.get(s, "~"), names[s], s)):
            if s not in new or s not in old:
                print(f"{names[s]:30s} {where.get(s, '-'):15s} {'':>5s} {'':>5s} {'':>6s} {'':>9s}  {'MISSING in the new units' if s not in new else 'NOT in the old unit'}  ({s})")
                ok = False
                continue
            o, n = old[s], new[s]
            same = o["body"] == n["body"] and o["desc"] == n["desc"]
            verdict = "identical" if same else "DIFFERENT"
            if not same and s in note:           # a renamed kernel that lost arguments: the size of its argument segment is the one line that may differ
                ka = lambda k: [l for l in k["body"] + k["desc"] if l.startswith(".amdhsa_kernarg_size")]
                rest_of = lambda k: [l for l in k["body"] + ["--"] + k["desc"] if not l.startswith(".amdhsa_kernarg_size")]
                if rest_of(o) == rest_of(n):
                    same, verdict = True, f"identical but for {ka(o)[0]} -> {ka(n)[0].split()[-1]}"
                    n_removed[1] += 1
            ok &= same
            anon = "_GLOBAL__N_" in s
            print(f"{names[s]:30s} {where[s]:15s} {n['vgpr']:5d} {n['sgpr']:5d} {n['lds']:6d} {n['scratch']:9d}  {verdict}"
                  f"{'' if anon else '  (outside the anonymous namespace)'}{'  (was ' + note[s] + ')' if s in note else ''}")
            if not same:
                for what in ("desc", "body"):
                    for d in list(difflib.unified_diff(o[what], n[what], "old", "new", lineterm="", n=1))[:40]:
                        print("#     " + d)
    for x in sorted(unused):
        print(f"# FAIL: --rename / --removed {x}: no such kernel in the old units")
        ok = False
    per = lambda counts: ", ".join(f"{u}.hip {k}" for u, k in counts.items())
    print(f"# {sum(n_old.values())} kernels in the old unit{'s (' + per(n_old) + ')' if len(n_old) > 1 else ''}, {sum(n_new.values())} in the new units ({per(n_new)})"
          f"{', ' + str(n_removed[0]) + ' more in the old units removed on purpose' if n_removed[0] else ''}: "
          + ("FAILED" if not ok else "ALL IDENTICAL" + (f" ({n_removed[1]} of them but for the size of the argument segment, as printed)" if n_removed[1] else "")))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
