#!/usr/bin/env python3
"""Diagnostic: instruction-class counts of a kernel in hipcc's assembly listing.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S www24-rat_amd/csrc/attn.hip -o attn.s
    python tools/isa_counts.py attn.s 'attn_bwd3_kernel<false, false, false, (false|true), 0, 8>'

The pattern is a regular expression searched in the kernel's mangled and demangled name.  For every kernel that matches it prints

  * the register budget from the code object's metadata: VGPRs, AGPRs, scratch bytes, VGPR / SGPR spills;
  * per barrier-delimited segment (the listing cut at every s_barrier, in listing order) and per innermost loop (a label with a
    backward branch to it and no other such loop inside) the number of instructions of each class:

      mfma    matrix-pipe instructions (v_mfma_*, v_smfmac_*)
      pk32    packed fp32 arithmetic (v_pk_fma_f32, v_pk_mul_f32, v_pk_add_f32)
      fp32    other fp32 arithmetic (v_fma_f32, v_mul_f32, v_add_f32, v_sub_f32, v_fmac_f32, v_max_f32, ...)
      cvt     conversions (v_cvt_*)
      trans   transcendentals (v_exp_*, v_log_*, v_rcp_*, v_rsq_*, v_sqrt_*, v_sin_*, v_cos_*)
      int     every other vector-ALU instruction: integer arithmetic, compares, selects, moves, lane reads
      valu    the sum of the six classes above
      ldsr    LDS reads (ds_read*, ds_load*)
      ldsw    LDS writes (ds_write*, ds_store*)
      gld     global loads (global_load*, buffer_load*, flat_load*)

The listing order of the blocks is the compiler's, not the program's: a segment is what stands between two barriers in the text.
Never used by the product or the tests."""
import re
import shutil
import subprocess
import sys

CLASSES = ("mfma", "pk32", "fp32", "cvt", "trans", "int", "valu", "ldsr", "ldsw", "gld")
TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")


def classify(op):
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "ldsr"
    if op.startswith("ds_write") or op.startswith("ds_store"):
        return "ldsw"
    if op.startswith(("global_load", "buffer_load", "flat_load")):
        return "gld"
    if not op.startswith("v_"):
        return None
    if op.startswith(("v_mfma_", "v_smfmac_")):
        return "mfma"
    if op.startswith("v_cvt_"):
        return "cvt"
    if op.startswith(TRANS):
        return "trans"
    if re.match(r"v_pk_(fma|mul|add)_f32", op):
        return "pk32"
    if re.match(r"v_(fma|fmac|mul|add|sub|subrev|mac|mad|max|min|max3|min3|med3|fmaak|fmamk|ldexp|fract|floor|ceil|trunc|rndne)_(legacy_)?f32", op):
        return "fp32"
    return "int"


def count(ops):
    c = dict.fromkeys(CLASSES, 0)
    for op in ops:
        k = classify(op)
        if k is not None:
            c[k] += 1
            if k in ("mfma", "pk32", "fp32", "cvt", "trans", "int"):
                c["valu"] += 1
    return c


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def functions(lines):
    """name -> (first line, last line) of every function body in the listing"""
    out, name, start = {}, None, 0
    for n, ln in enumerate(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):\s*;\s*@", ln)
        if m:
            name, start = m.group(1), n + 1
        elif name is not None and ln.startswith(".Lfunc_end"):
            out[name] = (start, n)
            name = None
    return out


def metadata(lines):
    """kernel name -> {key: value} from the amdhsa.kernels list of the metadata note"""
    out, cur = {}, None
    for ln in lines:
        m = re.match(r"^\s+(- )?\.(\w+):\s*(.*)$", ln)
        if not m:
            continue
        if m.group(1) and re.match(r"^  - ", ln):
            cur = {}
        if cur is not None:
            cur[m.group(2)] = m.group(3).strip()
            if m.group(2) == "name":
                out[m.group(3).strip()] = cur
    return out


def body(lines, lo, hi):
    """[(label or None, mnemonic or None, branch target or None)] of the function's label and instruction lines"""
    out = []
    for ln in lines[lo:hi]:
        s = ln.split(";")[0].rstrip()
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            out.append((m.group(1), None, None))
            continue
        m = re.match(r"^\s+([a-z]\w*)\s*(.*)$", s)
        if m and not s.lstrip().startswith("."):
            op, rest = m.group(1), m.group(2)
            tgt = rest.strip() if op.startswith(("s_cbranch", "s_branch")) else None
            out.append((None, op, tgt))
    return out


def report(name, pretty, items, meta):
    print("kernel %s" % pretty)
    if meta:
        print("  vgprs %s  agprs %s  scratch bytes %s  vgpr spills %s  sgpr spills %s" % (
            meta.get("vgpr_count", "?"), meta.get("agpr_count", "?"), meta.get("private_segment_fixed_size", "?"),
            meta.get("vgpr_spill_count", "?"), meta.get("sgpr_spill_count", "?")))
    head = "  %-22s" % "" + "".join("%6s" % k for k in CLASSES)
    # segments
    seg_of, seg, segs = [], 0, [[]]
    for lab, op, _ in items:
        seg_of.append(seg)
        if op is not None:
            segs[-1].append(op)
            if op == "s_barrier":
                seg += 1
                segs.append([])
    print(head)
    tot = dict.fromkeys(CLASSES, 0)
    for k, ops in enumerate(segs):
        c = count(ops)
        for key in CLASSES:
            tot[key] += c[key]
        print("  %-22s" % ("segment %d" % k) + "".join("%6d" % c[key] for key in CLASSES))
    print("  %-22s" % "whole kernel" + "".join("%6d" % tot[key] for key in CLASSES))
    # loops: backward branches
    pos = {lab: n for n, (lab, _, _) in enumerate(items) if lab is not None}
    spans = sorted({(pos[t], n) for n, (_, _, t) in enumerate(items) if t in pos and pos[t] < n})
    heads = {}
    for lo, hi in spans:                                   # several back edges to one label: the loop is the longest span
        heads[lo] = max(hi, heads.get(lo, 0))
    spans = sorted(heads.items())
    inner = [(lo, hi) for lo, hi in spans if not any((a, b) != (lo, hi) and lo <= a and b <= hi for a, b in spans)]
    print("  innermost loops (label, segment, instructions of all kinds):")
    for lo, hi in inner:
        ops = [op for _, op, _ in items[lo:hi + 1] if op is not None]
        c = count(ops)
        print("  %-22s" % ("%s s%d n%d" % (items[lo][0], seg_of[lo], len(ops))) + "".join("%6d" % c[key] for key in CLASSES))
    print()


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    lines = open(sys.argv[1]).read().split("\n")
    pat = re.compile(sys.argv[2])
    funcs = functions(lines)
    meta = metadata(lines)
    pretty = demangle(sorted(funcs))
    hit = [n for n in funcs if n in meta and (pat.search(n) or pat.search(pretty[n]))]
    if not hit:
        sys.exit("no kernel matches %r" % sys.argv[2])
    for n in sorted(hit, key=lambda n: pretty[n]):
        report(n, pretty[n], body(lines, *funcs[n]), meta[n])


if __name__ == "__main__":
    main()
