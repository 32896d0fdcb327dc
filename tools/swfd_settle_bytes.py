"""Bytes the row movers of a sketch rotation store, counted from the shapes and from the counters of a lane-batched sketch
at config-2 shapes in its second epoch (as tools/profile_sketch.py): after every rotation of the second window the kept-row
counts (meta), the rows in use before the rotation (mused_swfd_debug_used) and the representatives (rep < 0: frozen) are
read back, and the rows each kernel writes follow from them:

    scatter + append (MUSED_SWFD_SETTLE=0)   live sketch: 2 l rows (kept rows, zeros to row 2 l) + l appended rows
    settle kernel                            live sketch: nk kept + l next rows + max(used - nk - l, 0) zero rows
    settle kernel, shared pending rows       live sketch: nk kept rows; every lane: the l next rows, once (the default)
    all of them                              frozen sketch: the l raw rows; dumped directions: one ring row each (not counted)
                                             (a level that freezes is written out once in the shared mode: not counted)

argv: lanes [rotations of the second window].  Prints one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mused_amd import _lib, synth
from mused_amd.swfd import SeqBasedSWFD

W, d, ell = 10000, 1024, 128
B = int(sys.argv[1]) if len(sys.argv) > 1 else 7
rots = int(sys.argv[2]) if len(sys.argv) > 2 else 78
X = torch.from_numpy(np.stack([np.concatenate([synth.stream_window("blob", 2 * t, W, d, 0)[0],
                                               synth.stream_window("blob", 2 * t + 1, W, d, 0)[0][:rots * ell]])
                               for t in range(B)])).cuda()
sk = SeqBasedSWFD(N=W, R=5500.0, d=d, sketch_dim=ell, lanes=B)
S = B * 2 * sk.L
L = _lib.lib()
for name in ("mused_swfd_debug_state", "mused_swfd_debug_used"):
    getattr(L, name).restype = C.c_int
    getattr(L, name).argtypes = [C.c_void_p] * 3 if name.endswith("state") else [C.c_void_p] * 2
sk.fit_lanes(X[:, :W])
rep, meta, used = (C.c_int * S)(), (C.c_int * (4 * S))(), (C.c_int * S)()
row = 8 * d
per = {"pair": [], "settle": [], "shared": [], "live": [], "frozen": [], "nk": [], "used": []}
for k in range(rots):
    sk.fit_lanes(X[:, W + k * ell:W + (k + 1) * ell])      # one block a call: the counters after every rotation
    assert L.mused_swfd_debug_state(sk._h, rep, meta) == 1 and L.mused_swfd_debug_used(sk._h, used) == 1
    r, nk, us = np.array(rep), np.array(meta).reshape(S, 4)[:, 0], np.array(used)
    live = r >= 0
    zero = np.maximum(us - nk - ell, 0)
    per["pair"].append(int(live.sum()) * 3 * ell * row + int((~live).sum()) * ell * row)
    per["settle"].append(int((nk + ell + zero)[live].sum()) * row + int((~live).sum()) * ell * row)
    per["shared"].append(int(nk[live].sum()) * row + B * ell * row + int((~live).sum()) * ell * row)
    per["live"].append(int(live.sum()))
    per["frozen"].append(int((~live).sum()))
    per["nk"].append(float(nk[live].mean()))
    per["used"].append(float(us[live].mean()))
sk.close()
mb = lambda v: round(float(np.mean(v)) / 2 ** 20, 1)
print(json.dumps({"lanes": B, "sketches": S, "rotations": rots, "live_mean": float(np.mean(per["live"])),
                  "frozen_mean": float(np.mean(per["frozen"])), "kept_rows_mean": round(float(np.mean(per["nk"])), 1),
                  "rows_in_use_before_mean": round(float(np.mean(per["used"])), 1),
                  "MB_stored_per_rotation_scatter_plus_append": mb(per["pair"]), "MB_stored_per_rotation_settle": mb(per["settle"]),
                  "MB_stored_per_rotation_settle_shared": mb(per["shared"]),
                  "MB_first_last_rotation_settle": [mb(per["settle"][:1]), mb(per["settle"][-1:])]}))
