#!/usr/bin/env python3
"""Static instruction counts of kernels in the assembly that `hipcc -save-temps` leaves (*-gfx950.s): per kernel whose
demangled-looking symbol contains every given substring, the vector-ALU, LDS, vector-memory and scalar instruction counts
of its body and the resources its metadata states (VGPRs, scratch, static LDS).  Counts are of the program text, not of
what a run executes: loops count once.

    tools/asm_counts.py k_forward-hip-amdgcn-amd-amdhsa-gfx950.s fwd_rows2_kernel
"""
import re
import subprocess
import sys


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return r.stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        return names


def kernels(path):
    """{symbol: [instruction lines]} for every .amdhsa kernel of the file, and {symbol: metadata dict}"""
    body, meta, cur = {}, {}, None
    desc = None
    with open(path) as f:
        for line in f:
            s = line.strip()
            m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", s)
            if m and not s.startswith(".L"):
                cur = m.group(1)
                body.setdefault(cur, [])
                continue
            if s.startswith(".amdhsa_kernel "):
                desc = s.split()[1]
                meta.setdefault(desc, {})
                cur = None
                continue
            if s.startswith(".end_amdhsa_kernel"):
                desc = None
                continue
            if desc and s.startswith(".amdhsa_"):
                k, _, v = s.partition(" ")
                meta[desc][k[len(".amdhsa_"):]] = v.strip()
                continue
            if s.startswith(".end_function") or s.startswith(".Lfunc_end"):
                cur = None
                continue
            if cur and s and not s.startswith((".", ";", "//")) and not s.endswith(":"):
                body[cur].append(s.split(";")[0].strip())
            # the comment block behind a kernel: "; NumVgprs: 68" and friends
            m = re.match(r"^;\s*(NumVgprs|NumAgprs|ScratchSize|LDSByteSize|Occupancy|TotalNumVgprs):\s*(\S+)", s)
            if m and desc is None:
                last = list(body)[-1] if body else None
                if last:
                    meta.setdefault(last, {})[m.group(1)] = m.group(2)
    return {k: v for k, v in body.items() if k in meta and v}, meta


def classify(ins):
    op = ins.split()[0]
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_"):
        return "salu"
    return "other"


def main():
    path, subs = sys.argv[1], sys.argv[2:]
    body, meta = kernels(path)
    syms = sorted(body)
    for sym, name in zip(syms, demangle(syms)):
        if not all(s in name for s in subs):
            continue
        c = {}
        for ins in body[sym]:
            k = classify(ins)
            c[k] = c.get(k, 0) + 1
        lds_w = sum(1 for i in body[sym] if i.startswith("ds_write") or i.startswith("ds_store"))
        m = meta[sym]
        print(name)
        print("  valu %d  mfma %d  lds %d (stores %d)  vmem %d  salu %d  total %d" %
              (c.get("valu", 0), c.get("mfma", 0), c.get("lds", 0), lds_w, c.get("vmem", 0), c.get("salu", 0), len(body[sym])))
        print("  vgprs %s  agprs %s  scratch %s  static lds %s  occupancy %s" %
              (m.get("NumVgprs", m.get("next_free_vgpr", "?")), m.get("NumAgprs", "?"),
               m.get("ScratchSize", m.get("private_segment_fixed_size", "?")), m.get("LDSByteSize", m.get("group_segment_fixed_size", "?")),
               m.get("Occupancy", "?")))


if __name__ == "__main__":
    main()
