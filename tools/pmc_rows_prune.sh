#!/bin/bash
# LDS bank conflicts, LDS activity and vector instructions per wave of the row kernel: one --pmc pass over a light bench
# run (stages launched whole), as tools/pmc_rows_conflicts.sh with two more counters.  The environment reaches the handle,
# so `HPFW_PRUNE=0 tools/pmc_rows_prune.sh` counts the kernel that forms every output of the last group.
# Output directory: $PMC_OUT (default out/pmc_rows_prune), removed afterwards.
cd "$(dirname "$0")/.."
export TMPDIR=/tmp HPFW_FWD_CHUNK=0
D="${PMC_OUT:-out/pmc_rows_prune}"
rm -rf "$D" && mkdir -p "$D"
rocprofv3 --kernel-trace --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_WAVES -d "$D" -o p --output-format csv -- python3 bench.py --no-parity --no-cpu-baseline --no-pcie --no-any-length --no-learn --no-search --no-stream --no-ffi --no-f32-chain --steps 2 --warmup 1 --batch 1000 > "$D/bench.log" 2>&1
python3 - "$D" <<'PY'
import csv, glob, collections, sys
f = glob.glob(sys.argv[1] + "/**/*_counter_collection.csv", recursive=True)[0]
acc = collections.defaultdict(lambda: collections.defaultdict(float))
for r in csv.DictReader(open(f)):
    k = r["Kernel_Name"]
    if "fwd_rows2" in k or "cq_kernel<12288" in k or "cq_kernel<6144" in k:
        acc[(k.split("(")[0][-60:], int(r["Grid_Size"]))][r["Counter_Name"]] += float(r["Counter_Value"])
for (k, g), d in sorted(acc.items(), key=lambda kv: -kv[0][1])[:6]:
    print(k, g, "conflict fraction %.3f" % (d["SQ_LDS_BANK_CONFLICT"] / max(d["SQ_LDS_IDX_ACTIVE"], 1)), "lds busy %.3f" % (d["SQ_LDS_IDX_ACTIVE"] / max(d["SQ_BUSY_CYCLES"], 1) / 8),
          "valu insts per wave %.1f" % (d["SQ_INSTS_VALU"] / max(d["SQ_WAVES"], 1)), "lds idx active %.4g" % d["SQ_LDS_IDX_ACTIVE"])
PY
rm -rf "$D"
