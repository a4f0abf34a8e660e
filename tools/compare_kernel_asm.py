#!/usr/bin/env python3
"""Compare the gfx950 code of two builds of csrc kernel by kernel (no GPU needed).

    make -C monopsr_amd/csrc EXTRA=-save-temps=obj        # in each of the two trees
    python tools/compare_kernel_asm.py OLD/monopsr_amd/csrc NEW/monopsr_amd/csrc [--diff]

Reads every *-gfx950.s that -save-temps left in the two directories and prints one line per kernel: `same` when the
instruction sequence, the kernel descriptor (.amdhsa_* directives: register counts, LDS, scratch, ...) and the metadata
entry (.vgpr_count, .agpr_count, .group_segment_fixed_size, .private_segment_fixed_size, spill counts, ...) are equal
after normalising what cannot matter:
  * kernels are matched by their demangled name without the parameter list, so a renamed parameter struct or a moved
    template does not unpair them (llvm-cxxfilt / c++filt; the mangled name itself where neither is found);
  * local labels (.LBB12_3) are renumbered in order of appearance;
  * comments, .file / .ident / .loc / .cfi and other directives inside a body are dropped.
The kernel-argument size and the argument list are reported apart (`kernarg A -> B`): they follow the parameter struct,
not the code.  --diff prints the normalised diff of every kernel that is not `same`.  Exit status 1 if any differs.
"""
import argparse
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys


def demangle(names):
    tool = next((t for t in ("/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt"))
                 if t and os.path.exists(t)), None)
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    res = {}
    for n, d in zip(names, out):
        # drop the parameter list: the last balanced (...) of the demangled name
        depth, cut = 0, len(d)
        for i in range(len(d) - 1, -1, -1):
            depth += d[i] == ")"
            depth -= d[i] == "("
            if depth == 0 and d[i] == "(":
                cut = i
                break
            if depth == 0 and d[i] != ")":
                break
        res[n] = re.sub(r"^void ", "", d[:cut]) or n
    return res


def kernels_of(path):
    """key -> dict(code=[...], desc=[...], meta={...}, kernarg=str) for every kernel of one .s file"""
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    keys = demangle(names)
    out = {}
    meta_text = text[text.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in text else ""
    meta_blocks = {}
    for blk in re.split(r"\n  - ", meta_text)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m:
            meta_blocks[m.group(1)] = blk
    for name in names:
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S).group(1)
        labels, code = {}, []

        def label(m):
            return labels.setdefault(m.group(0), ".L%d" % len(labels))

        for line in body.split("\n"):
            t = line.split(";")[0].strip()
            if not t or (t.startswith(".") and not t.endswith(":")):
                continue
            t = re.sub(r"\.L[A-Za-z_]*\d+(?:_\d+)?", label, t)
            for n2 in names:
                t = t.replace(n2, "<%s>" % keys[n2])
            code.append(" ".join(t.split()))
        desc = re.search(r"\.amdhsa_kernel\s+%s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), text, re.S).group(1)
        desc = [" ".join(l.split(";")[0].split()) for l in desc.split("\n") if l.strip()]
        blk = meta_blocks.get(name, "")
        meta = dict(re.findall(r"^\s+(\.(?!name|symbol|args|kernarg_segment_size)\w+):\s+(\S+)\s*$", blk, re.M))
        for k in [k for k in meta if k.startswith((".offset", ".size", ".value_kind", ".address_space", ".actual_access"))]:
            del meta[k]
        kernarg = re.search(r"\.kernarg_segment_size:\s+(\d+)", blk)
        desc = [l for l in desc if not l.startswith(".amdhsa_kernarg_size")]
        out[keys[name]] = dict(code=code, desc=desc, meta=meta, kernarg=kernarg.group(1) if kernarg else "?")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--diff", action="store_true", help="print the normalised diff of every kernel that differs")
    a = ap.parse_args()
    suffix = "-hip-amdgcn-amd-amdhsa-gfx950.s"
    files = {}
    for side, d in (("old", a.old), ("new", a.new)):
        for p in glob.glob(os.path.join(d, "*" + suffix)):
            files.setdefault(os.path.basename(p)[:-len(suffix)], {})[side] = p
    bad = 0
    for stem in sorted(files):
        if len(files[stem]) != 2:
            print("%s.hip: only in the %s build" % (stem, next(iter(files[stem]))))
            bad += 1
            continue
        old, new = kernels_of(files[stem]["old"]), kernels_of(files[stem]["new"])
        for key in sorted(set(old) | set(new)):
            if key not in old or key not in new:
                print("%s.hip  %s: only in the %s build" % (stem, key, "old" if key in old else "new"))
                bad += 1
                continue
            o, n = old[key], new[key]
            what = []
            if o["code"] != n["code"]:
                what.append("code differs (%d -> %d instructions and labels)" % (len(o["code"]), len(n["code"])))
            if o["desc"] != n["desc"]:
                what.append("descriptor differs")
            if o["meta"] != n["meta"]:
                what.append("metadata differs: " + ", ".join(
                    "%s %s -> %s" % (k, o["meta"].get(k), n["meta"].get(k))
                    for k in sorted(set(o["meta"]) | set(n["meta"])) if o["meta"].get(k) != n["meta"].get(k)))
            karg = "" if o["kernarg"] == n["kernarg"] else "  [kernarg %s -> %s bytes]" % (o["kernarg"], n["kernarg"])
            print("%s.hip  %s: %s%s" % (stem, key, "; ".join(what) if what else
                                        "same (%d instructions, vgpr %s agpr %s lds %s scratch %s)" % (
                                            sum(not c.endswith(":") for c in n["code"]), n["meta"].get(".vgpr_count"),
                                            n["meta"].get(".agpr_count"), n["meta"].get(".group_segment_fixed_size"),
                                            n["meta"].get(".private_segment_fixed_size")), karg))
            if what:
                bad += 1
                if a.diff:
                    for part in ("code", "desc"):
                        sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(
                            o[part], n[part], "old/" + key, "new/" + key, lineterm="", n=2))
    print("%d kernel(s) differ" % bad if bad else "all kernels same")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
