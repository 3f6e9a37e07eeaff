#!/usr/bin/env python3
"""Per-kernel comparison of two builds of a .hip file, without a GPU.

For each side, compile with
    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S \
          -Rpass-analysis=kernel-resource-usage F.hip -o DIR/F.s 2> DIR/F.remarks
then  isa_compare.py OLD_DIR NEW_DIR F [F ...]

Counts the fp64 fma / mul / add instructions (scalar and packed forms) of every kernel symbol and
reads the compiler's resource remarks.  Exit status 1 if a kernel's counts or LDS size differ, its
scratch or spills grow, or its occupancy drops.
"""
import re
import sys
from collections import Counter

CLASSES = {
    "fma": ("v_fma_f64", "v_fmac_f64"), "pk_fma": ("v_pk_fma_f64",),
    "mul": ("v_mul_f64",), "pk_mul": ("v_pk_mul_f64",),
    "add": ("v_add_f64",), "pk_add": ("v_pk_add_f64",),
}
REMARKS = {"TotalSGPRs": "sgpr", "VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch",
           "Occupancy [waves/SIMD]": "occ", "SGPRs Spill": "sspill", "VGPRs Spill": "vspill",
           "LDS Size [bytes/block]": "lds"}


def read_asm(path):
    """{kernel symbol: (Counter of instruction classes, body lines)}"""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None and line.startswith(".Lfunc_end"):
            cnt = Counter()
            for b in body:
                op = b.split()[0] if b.split() else ""
                op = re.sub(r"_e(32|64)$|_dpp$", "", op)
                for cls, ops in CLASSES.items():
                    if op in ops:
                        cnt[cls] += 1
            out[name] = (cnt, body)
            name = None
            continue
        if name is not None:
            body.append(line.strip())
    return out


def read_remarks(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(": ")
        if key == "Function Name":
            name = val
            out[name] = {}
        elif key in REMARKS and name is not None:
            out[name][REMARKS[key]] = int(val)
    return out


def main(old_dir, new_dir, files):
    bad = 0
    for f in files:
        a, b = read_asm(f"{old_dir}/{f}.s"), read_asm(f"{new_dir}/{f}.s")
        ra, rb = read_remarks(f"{old_dir}/{f}.remarks"), read_remarks(f"{new_dir}/{f}.remarks")
        kernels = sorted(ra)
        assert kernels == sorted(rb) and all(k in a and k in b for k in kernels), f
        same_text = sum(a[k][1] == b[k][1] for k in kernels)
        print(f"## {f}.hip: {len(kernels)} kernels, {same_text} with identical assembly\n")
        lines = []
        for k in kernels:
            rows = [(c, a[k][0][c], b[k][0][c], a[k][0][c] == b[k][0][c]) for c in CLASSES]
            x, y = ra[k], rb[k]
            rows.append(("lds", x["lds"], y["lds"], x["lds"] == y["lds"]))
            for key in ("scratch", "sspill", "vspill"):
                rows.append((key, x[key], y[key], y[key] <= x[key]))
            rows.append(("occ", x["occ"], y["occ"], y["occ"] >= x["occ"]))
            for key in ("vgpr", "agpr", "sgpr"):
                rows.append((key, x[key], y[key], True))
            for what, p, c, ok in rows:
                if p != c:
                    lines.append(f"| `{k}` | {what} | {p} | {c} | {'' if ok else 'FAIL'} |")
                bad += not ok
        if lines:
            print("\n".join(["| kernel | what | parent | change | |", "|---|---|---|---|---|"] + lines))
        else:
            print("no kernel differs in a count or a resource figure")
        tot = Counter()
        for k in kernels:
            tot.update(b[k][0])
        print(f"\nfp64 instructions of the change, all kernels: {dict(tot)}\n")
    print("verdict:", "FAIL" if bad else "ok", f"({bad} violations)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
