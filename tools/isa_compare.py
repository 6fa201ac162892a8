#!/usr/bin/env python3
"""Compare the device assembly of the row-owning kernels between two commits, kernel by kernel, as text.

    python tools/check_rowgemm_isa.py --keep-asm=DIR      (once at each commit: DIR/<source file>/<mangled name>.s)
    python tools/isa_compare.py PARENT_DIR NEW_DIR [--out=FILE.md]

Writes the table of profiles/rowtail_isa.md and profiles/row_mainloop_isa.md.  Per source file: the kernels whose text is
identical; the kernels that differ but keep the parent's instruction mix, main-loop instruction counts and footprint, as a list
with two figures each -- how many instruction lines differ as text (difflib, both sides counted), and how many still differ
once every register number is masked (v12, s[4:5], a3 -> v, s, a: 0 = register names only, in the same order); and for each
other kernel those two figures and
  * lines parent / new (instructions: labels, directives, comments and blank lines are not counted);
  * whether the instruction mix (how often each mnemonic occurs) is the same;
  * the main loops' instruction counts parent / new -- a loop being the text between a label and the last backward branch
    to it, a main loop one that holds MFMAs and no other loop -- in program order;
  * how the instruction mix differs, mnemonic by mnemonic (parent -> new);
  * the footprint parent / new: next free VGPR / accum offset / next free SGPR / scratch bytes / static LDS bytes.
One normalisation, nothing else: basic-block labels (.LBB<f>_<n>, and BB<f>_<n> in comments) carry the index <f> of the
function in its file, which moves when the host code instantiates the kernels in another order; <f> is dropped on both sides.
Kernels present on one side only are listed as such.  Exit code 0 whatever the texts say: the tool reports, it asserts nothing."""
import collections
import difflib
import os
import re
import shutil
import subprocess
import sys

FOOT = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")
LABEL = re.compile(r"\bBB\d+_(\d+)")


def normalise(text):
    return LABEL.sub(r"BB_\1", text)


def instructions(text):
    """the instruction lines of a kernel's text (up to its s_endpgm), labels kept as 'name:'"""
    out = []
    for ln in text.split(".amdhsa_kernel")[0].split("\n"):
        t = ln.split(";")[0].strip()
        if not t or t.startswith(".") and not t.endswith(":"):
            continue
        out.append(t)
    return out


def loops(ins):
    """[instruction count] of every innermost loop (label .. last backward branch to it) that holds MFMAs, in program order"""
    at = {t[:-1]: i for i, t in enumerate(ins) if t.endswith(":")}
    last = {}
    for i, t in enumerate(ins):
        parts = t.split()
        if parts[0].startswith(("s_cbranch", "s_branch")) and parts[-1] in at and at[parts[-1]] < i:
            last[parts[-1]] = i
    spans = sorted((at[l], last[l]) for l in last)
    inner = [(a, b) for a, b in spans if not any((c, d) != (a, b) and a <= c and d <= b for c, d in spans)]
    return [sum(1 for t in ins[a:b + 1] if not t.endswith(":")) for a, b in inner if any(t.startswith("v_mfma") for t in ins[a:b + 1])]


REGS = re.compile(r"\b([vsa])(\d+|\[\d+:\d+\])")


def differing(a, b):
    """instruction lines of a and of b outside difflib's matching blocks, added up"""
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    return len(a) + len(b) - 2 * sum(m.size for m in sm.get_matching_blocks())


def differing_lines(ip, inn):
    """'as text / with register numbers masked'"""
    masked = [[REGS.sub(r"\1", t) for t in ins] for ins in (ip, inn)]
    return f"{differing(ip, inn)} / {differing(*masked)}"


def footprint(text):
    d = dict(re.findall(r"\.amdhsa_(\w+)\s+(\d+)", text))
    return " / ".join(d.get(k, "?") for k in FOOT)


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True) if tool and names else None
    out = r.stdout.split("\n")[:len(names)] if r and r.returncode == 0 else names
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"^void\s+", "", d).replace("(anonymous namespace)::", "").split("(")[0].replace("jv::", "").replace(", ", ",")
        short[n] = re.sub(r"\((\w+)\)(\d+)", r"\2", d).replace("true", "1").replace("false", "0")
    return short


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 2:
        print(__doc__)
        return 2
    pdir, ndir = args
    out = sys.stdout
    for a in sys.argv[1:]:
        if a.startswith("--out="):
            out = open(a.split("=", 1)[1], "w")
    n_all = n_same = 0
    for src in sorted(set(os.listdir(pdir)) | set(os.listdir(ndir))):
        def read(d):
            p = os.path.join(d, src)
            return {f[:-2]: open(os.path.join(p, f)).read() for f in os.listdir(p) if f.endswith(".s")} if os.path.isdir(p) else {}
        par, new = read(pdir), read(ndir)
        names = sorted(set(par) | set(new))
        short = demangle(names)
        both = [n for n in names if n in par and n in new]
        same = [n for n in both if normalise(par[n]) == normalise(new[n])]
        diff = [n for n in both if n not in same]
        n_all += len(both)
        n_same += len(same)
        print(f"## {src}: {len(both)} kernels, {len(same)} identical, {len(diff)} differing\n", file=out)
        for side, only in (("parent", set(par) - set(new)), ("new", set(new) - set(par))):
            if only:
                print(f"Only in the {side} build: " + ", ".join(f"`{short[n]}`" for n in sorted(only)) + "\n", file=out)
        if same:
            print("Identical: " + ", ".join(f"`{short[n]}`" for n in sorted(same, key=short.get)) + "\n", file=out)
        rows, quiet = [], []
        for n in sorted(diff, key=short.get):
            ip, inn = instructions(par[n]), instructions(new[n])
            mp = collections.Counter(t.split()[0] for t in ip if not t.endswith(":"))
            mn = collections.Counter(t.split()[0] for t in inn if not t.endswith(":"))
            what = ", ".join(f"{m} {mp[m]} -> {mn[m]}" for m in sorted(set(mp) | set(mn)) if mp[m] != mn[m])
            lp, ln_ = loops(ip), loops(inn)
            fp, fn = footprint(par[n]), footprint(new[n])
            dl = differing_lines(normalise("\n".join(ip)).split("\n"), normalise("\n".join(inn)).split("\n"))
            if mp == mn and lp == ln_ and fp == fn:
                quiet.append(f"`{short[n]}` ({dl})")      # (the same mix implies the same line count)
                continue
            lo = ("same: " if lp == ln_ else "DIFFER: ") + (" ".join(map(str, lp)) or "-") + " / " + (" ".join(map(str, ln_)) or "-")
            rows.append(f"| `{short[n]}` | {sum(mp.values())} / {sum(mn.values())} | {dl} | {'yes' if mp == mn else 'NO'} | {lo} | {fp} | {fn} | {what} |")
        if quiet:
            print("Differing, with the parent's line count, instruction mix, main-loop instruction counts and footprint "
                  "(lines differing as text / with register numbers masked): " + ", ".join(quiet) + "\n", file=out)
        if rows:
            print("| kernel | lines parent / new | lines differing: text / masked | same instruction mix | main loops: parent / new | footprint parent | footprint new | mix: parent -> new |", file=out)
            print("|---|---|---|---|---|---|---|---|", file=out)
            print("\n".join(rows) + "\n", file=out)
    print(f"{n_same} of {n_all} kernels are identical text.", file=out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
