#!/usr/bin/env python3
"""Compare the gfx950 code of .hip files between two revisions, kernel by kernel.

  python scripts/isa_compare.py REV_A REV_B pilosa_amd/kernels/pair_kernels.hip
  python scripts/isa_compare.py REV_A REV_B PATHS_A [PATHS_B]

REV is anything `git archive` takes, or `.` for the working tree.  PATHS is a
comma-separated list of files whose kernels are pooled on that side (PATHS_B
defaults to PATHS_A); a file a revision does not have is skipped with a note.
So kernels can be followed across a file split:

  python scripts/isa_compare.py HEAD~1 . pilosa_amd/kernels/bitmap_kernels.hip,pilosa_amd/kernels/bsi_kernels.hip

Each side's kernel directory (so its own headers) goes to a temp directory and
is cross-compiled to assembly; no GPU is needed.  Per kernel the report says
whether the normalised text (comments stripped, .LBB labels renumbered) is
identical, and gives VGPRs / SGPRs / LDS / scratch before -> after, the
instruction count and the opcode-count delta.  Kernels are matched by their
demangled name; where a template's parameter list differs between the
revisions, TEMPLATE_KEYS names the parameters that identify an instantiation.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT", "c++filt")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S"]
# template name -> {number of template arguments: positions of the identifying ones}
TEMPLATE_KEYS = {"and2_pairs_v6_kernel": {11: (0, 6, 9), 3: (0, 1, 2), 4: (0, 1, 2, 3)}}   # (CQ, BST, TWN[, DQ])
# template name -> number of identifying arguments a revision without the later ones has: trailing
# arguments past it are dropped from the key while they are 0 (the instantiations that revision had)
TRAILING_FLAGS = {"and2_pairs_v6_kernel": 3}
RENAMED = {"shadow_build_kernel": "twin_build_kernel"}
STATS = (("vgpr", "NumVgprs"), ("sgpr", "TotalNumSgprs"), ("lds", "LDSByteSize"), ("scratch", "ScratchSize"))


def assembly(rev, paths, tmp):
    """{path: assembly} of the listed files at rev; a file the revision does not have is skipped"""
    out = {}
    for n, path in enumerate(paths):
        src = os.path.dirname(path) or "."
        if rev != ".":
            src = os.path.join(tmp, "src%d" % n)
            os.makedirs(src)
            tar = subprocess.run(["git", "archive", rev, "--", os.path.dirname(path)], check=True, capture_output=True)
            subprocess.run(["tar", "-x", "--strip-components", str(path.count("/")), "-C", src], input=tar.stdout,
                           check=True)
        file = os.path.join(src, os.path.basename(path))
        if not os.path.exists(file):
            print("note: %s does not exist at %s, skipped" % (path, rev))
            continue
        asm = os.path.join(tmp, "out%d.s" % n)
        subprocess.run([HIPCC, *FLAGS, file, "-o", asm], check=True)
        out[path] = open(asm).read()
    return out


def key_of(mangled):
    name = subprocess.run([CXXFILT, mangled], check=True, capture_output=True, text=True).stdout.strip()
    m = re.match(r"(?:void )?(?:[\w:]|\(anonymous namespace\))*?(\w+)(?:<(.*?)>)?\(", name)
    base, args = m.group(1), [a.strip() for a in (m.group(2) or "").split(",") if a.strip()]
    pos = TEMPLATE_KEYS.get(base, {}).get(len(args))
    norm = {"false": "0", "true": "1"}
    args = [norm.get(args[p], args[p]) for p in pos] if pos else args
    while base in TRAILING_FLAGS and len(args) > TRAILING_FLAGS[base] and args[-1] == "0":
        args.pop()
    return RENAMED.get(base, base) + ("<" + ", ".join(args) + ">" if args else "")


def kernels(asm):
    """{key: (normalised instruction lines, {stat: value})} of every kernel in the assembly"""
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:\n(.*?)^; Occupancy", asm, re.M | re.S):
        if ".amdhsa_kernel " + m.group(1) not in asm:
            continue
        labels, lines = {}, []
        for ln in m.group(2).splitlines():
            ln = re.sub(r"\.LBB\d+_\d+", lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)),
                        ln.split(";")[0].strip())
            if ln and not ln.startswith("."):
                lines.append(ln)
            elif ln.endswith(":"):
                lines.append(ln)
        stats = {k: int(re.search(r"; %s: (\d+)" % tag, m.group(3)).group(1)) for k, tag in STATS}
        out[key_of(m.group(1))] = (lines, stats)
    return out


def opcodes(lines):
    return collections.Counter(ln.split()[0] for ln in lines if not ln.endswith(":"))


def pooled(rev, paths, tmp):
    out = {}
    for path, asm in assembly(rev, paths, tmp).items():
        for key, val in kernels(asm).items():
            if key in out:
                sys.exit("%s: kernel %s is in more than one of %s" % (rev, key, ", ".join(paths)))
            out[key] = val
    return out


def main():
    rev_a, rev_b = sys.argv[1:3]
    paths_a = sys.argv[3].split(",")
    paths_b = sys.argv[4].split(",") if len(sys.argv) > 4 else paths_a
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        a, b = pooled(rev_a, paths_a, ta), pooled(rev_b, paths_b, tb)
    print("%s @ %s -> %s @ %s (%s)" % (",".join(paths_a), rev_a, ",".join(paths_b), rev_b, " ".join(FLAGS)))
    same = 0
    for key in sorted(set(a) | set(b)):
        if key not in a or key not in b:
            print("%-40s only in %s" % (key, rev_a if key in a else rev_b))
            continue
        (la, sa), (lb, sb) = a[key], b[key]
        same += la == lb
        oa, ob = opcodes(la), opcodes(lb)
        na, nb = sum(oa.values()), sum(ob.values())
        print("%-40s %s  %s  insts %d -> %d" % (key, "identical" if la == lb else "DIFFERENT", "  ".join(
            "%s %d -> %d" % (k, sa[k], sb[k]) for k, _ in STATS), na, nb))
        delta = {op: ob[op] - oa[op] for op in sorted(set(oa) | set(ob)) if ob[op] != oa[op]}
        if delta:
            print("    opcode delta: " + ", ".join("%s %+d" % kv for kv in delta.items()))
    both = len(set(a) & set(b))
    print("%d of %d kernels identical, %d different, %d on one side only" % (
        same, len(set(a) | set(b)), both - same, len(set(a) ^ set(b))))


if __name__ == "__main__":
    main()
