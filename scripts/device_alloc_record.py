"""device_alloc_record.py [--tree DIR] [--out FILE]: the figures of profiles/device_alloc on one MI355X, from the library of a checkout (default: this one).

Per handle of tests/test_device_alloc_gpu.py: info()["a_bytes"] after creation and after one call of every entry, and the bytes of the fp8 image
(a8_info()["image_bytes"]); per training geometry 15 timed sgd_step and adam_step calls (dt_ms: the device time between the call's two events).  Uses
only entry points that exist on both sides of the refactor, so that --tree may name a checkout of the commit before it; the helpers come from this
checkout's tests/."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=ROOT)
ap.add_argument("--out", default=None)
args = ap.parse_args()
tree = os.path.abspath(args.tree)
sys.path[:0] = [tree, os.path.join(ROOT, "tests")]

import numpy as np
import torch
import sparta_amd as sa
import test_device_alloc_gpu as T

assert os.path.abspath(sa.__file__).startswith(tree), sa.__file__


class Env:
    """what open_handle asks of pytest's monkeypatch; undone below"""

    def __init__(self):
        self.saved = {}

    def setenv(self, k, v):
        self.saved.setdefault(k, os.environ.get(k))
        os.environ[k] = v

    def undo(self):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


out = {"bytes": {}, "sgd_ms": {}, "adam_ms": {}}
for name in T.HANDLES:
    env = Env()
    out["bytes"][name] = list(T.figures(torch, name, env))
    env.undo()
    print(name, out["bytes"][name], flush=True)
for name in T.HANDLES[:4]:
    h, W = T.open_handle(name)
    w = torch.from_numpy(W).cuda()
    g = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, W.size).astype(np.float32)).cuda()
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    s = torch.zeros(8, dtype=torch.int32, device="cuda")
    for _ in range(3):
        h.sgd_step(w, g, m, lr=1e-3, momentum=0.9)
        h.adam_step(w, g, m, v, s, lr=1e-3)
    torch.cuda.synchronize()
    out["sgd_ms"][name] = [h.sgd_step(w, g, m, lr=1e-3, momentum=0.9, timed=True) for _ in range(15)]
    out["adam_ms"][name] = [h.adam_step(w, g, m, v, s, lr=1e-3, timed=True) for _ in range(15)]
    h.close()
    print(name, "sgd", min(out["sgd_ms"][name]), max(out["sgd_ms"][name]), "adam", min(out["adam_ms"][name]), max(out["adam_ms"][name]), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
