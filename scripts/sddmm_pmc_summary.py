"""Per-launch counter means of the SDDMM kernels and of the forward product, from rocprofv3 --pmc passes of scripts/sddmm_record.py:

    for set in "FETCH_SIZE" "WRITE_SIZE TCC_HIT_sum TCC_MISS_sum" "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY" \\
               "SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_VMEM GRBM_GUI_ACTIVE" "SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_LDS SQ_INSTS_LDS"; do
      rocprofv3 --pmc $set --output-format csv -d OUT/<dtype>_<n> -o run -- python scripts/sddmm_record.py --dtype <dtype> --reps 10
    done
    python scripts/sddmm_pmc_summary.py OUT          -> OUT/pmc_summary.json (one entry per dtype and kernel)

The directory name before the first "_" is the dtype.  FETCH_SIZE / WRITE_SIZE are in KB as rocprofv3 reports them (on gfx950 FETCH_SIZE
reports half of a wide coalesced read: MI355X_MICROARCH.md, HBM)."""
import collections
import csv
import glob
import json
import os
import re
import sys


def main():
    out = sys.argv[1]
    agg = collections.defaultdict(lambda: collections.defaultdict(list))
    dur = collections.defaultdict(list)
    for f in sorted(glob.glob(os.path.join(out, "*", "**", "*counter_collection.csv"), recursive=True)):
        dt = os.path.relpath(f, out).split(os.sep)[0].split("_")[0]
        for r in csv.DictReader(open(f)):
            m = re.search(r"vbs_(sddmm|spmm)\w*", r["Kernel_Name"])
            if not m:
                continue
            key = (dt, m.group(0))
            agg[key][r["Counter_Name"]].append(float(r["Counter_Value"]))
            dur[key].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    res = {}
    for (dt, name), d in sorted(agg.items()):
        e = {c: round(sum(v) / len(v), 1) for c, v in sorted(d.items())}
        e["dispatches"] = max(len(v) for v in d.values())
        e["profiled_us"] = round(sum(dur[(dt, name)]) / len(dur[(dt, name)]) / 1e3, 2)
        res.setdefault(dt, {})[name] = e
    json.dump(res, open(os.path.join(out, "pmc_summary.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
