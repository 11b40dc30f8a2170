"""Are two `hipcc --cuda-device-only -S` outputs of one source the same kernels, whatever ORDER they were emitted in?

    python tools/asm_same_kernels.py PARENT.s TREE.s [--rename REGEX REPLACEMENT]        exit status 0: yes

A host-side edit that changes the order in which kernel templates are first referenced changes the order in which the compiler
emits them, and with it the ordinal inside every local label (.LBB<n>_<m>, .Lfunc_end<n>): a plain diff then shows most of the
file although no instruction moved.  This splits both files at the kernels' `.section .text.<symbol>` lines, replaces the ordinal
in local labels (and in the comments that quote them), squeezes the blanks that pad those comments, and compares the kernels by
symbol; the metadata entries (one per kernel) are compared as a set, and everything outside kernels line by line, where only the
compilation-unit id (__hip_cuid_) may differ.  Printed: the kernel counts, how many kernels differ in text, how many positions
hold another kernel than in the first file, and the differing lines outside kernels.

--rename REGEX REPLACEMENT (re.sub, so \\1 names a group) is applied to the whole text of the FIRST file before it is parsed: an edit that
drops or adds a template parameter changes the mangled names and nothing else, and the parent's symbols - in labels, directives,
comments and metadata alike - are rewritten to the tree's mangling so that the kernels pair up.  The dropped `bool STAGE` of
gemm16_mfma_kernel:   --rename '(gemm16_mfma_kernelILi[0-9]*ELi[0-9]*ELi[0-9]*E)Lb1E' '\\1'"""
import argparse
import re
import sys


def parse(path, rename=None):
    text = open(path).read()
    if rename:
        text = re.sub(rename[0], rename[1], text)
    lines = text.split("\n")
    meta_a, meta_b = lines.index("\t.amdgpu_metadata"), lines.index("\t.end_amdgpu_metadata")
    body, meta = lines[:meta_a], lines[meta_a:meta_b + 1]
    begins = [i for i, l in enumerate(body) if "; -- Begin function" in l]
    for pattern in (r"\s*\.protected\s", r"\s*\.section\s+\.text\."):  # the two lines that may stand ahead of `.globl`
        begins = [i - 1 if re.match(pattern, body[i - 1]) else i for i in begins]
    end = next(i for i, l in enumerate(body) if ".AMDGPU.gpr_maximums" in l)
    kernels, order = {}, []
    for n, b0 in enumerate(begins):
        block = body[b0:begins[n + 1] if n + 1 < len(begins) else end]
        name = next(m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel (\S+)", l) for l in block) if m)
        assert name not in kernels, name
        kernels[name] = [re.sub(r" +", " ", re.sub(r"\bBB\d+_", "BBn_", re.sub(r"\.L([A-Za-z_]+)\d+", r".L\1n", l))) for l in block]
        order.append(name)
    entries, rest, cur = [], [], None
    for l in meta:
        if l.startswith("  - "):
            cur = [l]
            entries.append(cur)
        elif cur is not None and l.startswith("    "):
            cur.append(l)
        else:
            cur = None
            rest.append(l)
    outside = body[:begins[0]] + body[end:] + rest + lines[meta_b + 1:]
    return kernels, order, sorted("\n".join(e) for e in entries), outside


def main(a_path, b_path, rename=None):
    (ka, oa, ma, xa), (kb, ob, mb, xb) = parse(a_path, rename), parse(b_path)
    differing = sorted(k for k in ka if k in kb and ka[k] != kb[k])
    moved = sum(1 for x, y in zip(oa, ob) if x != y)
    outside = [(x, y) for x, y in zip(xa, xb) if x != y and "__hip_cuid_" not in x] + [None] * abs(len(xa) - len(xb))
    same = set(ka) == set(kb) and not differing and ma == mb and not outside
    print(f"{a_path} vs {b_path}: kernels {len(ka)} / {len(kb)}, same symbols {set(ka) == set(kb)}, kernels whose text differs "
          f"{len(differing)}, metadata entries equal {ma == mb}, positions holding another kernel {moved}, differing lines outside "
          f"kernels (unit id aside) {len(outside)}")
    for k in differing[:5]:
        print("  differs:", k)
    return 0 if same else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("first")
    ap.add_argument("second")
    ap.add_argument("--rename", nargs=2, metavar=("REGEX", "REPLACEMENT"), help="re.sub applied to the whole text of the first file")
    args = ap.parse_args()
    sys.exit(main(args.first, args.second, args.rename))
