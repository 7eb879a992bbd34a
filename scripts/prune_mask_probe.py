"""Where the time of DeviceVBS.mask_blocks goes, on the handle of scripts/prune_record.py (its method: event windows with the host side inside, arms interleaved
in a seeded order, [median, p10, p90] of 50 calls, ms): three tensors / one tensor with every second block, every block, no block, the first half of the blocks
pruned; hipMemsetAsync of the same bytes; torch's zero_(); and the kernels alone, through the entries' own dt_ms (events recorded in C around the launch).
One JSON line (profiles/prune/mask_probe.json).

    python scripts/prune_mask_probe.py"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import sparta_amd as sa  # noqa: E402
from prune_record import hip_runtime  # noqa: E402

w = 32
m = sa.gen.cant_like(seed=2)
eng = sa.BlockingEngine(blocking_algo=5, tau=0.6, col_block_size=w, row_block_size=32, force_fixed_size=True, sim_measure=1)
vb = sa.VBR().fill_from_CSR_inplace(m, eng.GetGrouping(m), w, 32, True)
nz, T = int(vb.nztot), vb.block_table()
nb = len(T)
H = vb.to_device(0, updatable=True)
Ts = [torch.ones(nz, device="cuda") for _ in range(3)]
alt = torch.from_numpy((np.arange(nb) % 2).astype(np.uint8)).cuda()
none = torch.zeros(nb, dtype=torch.uint8, device="cuda")
kept = torch.ones(nb, dtype=torch.uint8, device="cuda")
first = torch.from_numpy((np.arange(nb) >= nb // 2).astype(np.uint8)).cuda()          # the first half pruned: one contiguous range per tensor
hip = hip_runtime()
half_bytes = 4 * int(T[0::2, 2].sum())
target = torch.empty(4 * nz * 3, dtype=torch.uint8, device="cuda")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
arms = {"mask3_alt": lambda: H.mask_blocks(alt, *Ts), "mask3_all": lambda: H.mask_blocks(none, *Ts), "mask3_nothing": lambda: H.mask_blocks(kept, *Ts),
        "mask3_first_half": lambda: H.mask_blocks(first, *Ts), "mask1_alt": lambda: H.mask_blocks(alt, Ts[0]), "mask1_all": lambda: H.mask_blocks(none, Ts[0]),
        "memset_half3": lambda: hip.hipMemsetAsync(C.c_void_p(target.data_ptr()), 0, 3 * half_bytes, st),
        "memset_all3": lambda: hip.hipMemsetAsync(C.c_void_p(target.data_ptr()), 0, 3 * 4 * nz, st),
        "memset_half1": lambda: hip.hipMemsetAsync(C.c_void_p(target.data_ptr()), 0, half_bytes, st),
        "torch_zero_half3": lambda: target[:3 * half_bytes].zero_()}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _ in range(5):
    for k in arms:
        arms[k]()
torch.cuda.synchronize()
times = {k: [] for k in arms}
rng = np.random.default_rng(3)
for _ in range(50):
    for k in rng.permutation(list(arms)):
        e0.record(); arms[str(k)](); e1.record(); e1.synchronize()
        times[str(k)].append(e0.elapsed_time(e1))
out = {k: [round(float(np.median(t)), 5), round(float(np.percentile(t, 10)), 5), round(float(np.percentile(t, 90)), 5)] for k, t in times.items()}
for name, k in (("nothing", kept), ("alt", alt), ("all", none)):          # the kernel alone: events recorded in C around the launch (dt_ms)
    t = [H.mask_blocks(k, *Ts, timed=True) for _ in range(50)]
    out["kernel_only_mask3_" + name] = [round(float(np.median(t)), 5), round(float(np.percentile(t, 10)), 5), round(float(np.percentile(t, 90)), 5)]
t = [H.block_ssq(Ts[0], timed=True)[1] for _ in range(50)]
out["kernel_only_block_ssq"] = [round(float(np.median(t)), 5), round(float(np.percentile(t, 10)), 5), round(float(np.percentile(t, 90)), 5)]
out["half_bytes_per_tensor"] = half_bytes
out["nztot"] = nz
print(json.dumps(out))
