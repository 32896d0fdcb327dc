"""The timed lock-step of a benchmark run in a compact kernel trace (tools/trace_compact.py): which stream finishes last, and what
the main stream's kernels sum to per window.

    python tools/trace_region.py <compact csv[.gz]> [t0_ms t1_ms]

The main stream is the one that runs the SpMM of the eigenstep.  Its kernels come in phases separated by the synchronises of
bench.py (set-up, warm-up lock-steps, the timed lock-step); the last phase is the timed region unless t0 / t1 are given.  For
every busy stream the chain that starts with the region is followed to its first gap of more than 1.5 ms, the synchronise that
ends the timed region (the sketch streams go on with the halo lock-step behind it)."""
import collections
import gzip
import sys

import numpy as np

path = sys.argv[1]
op = gzip.open if path.endswith(".gz") else open
rows = [line.rstrip("\n").rsplit(",", 6) for i, line in enumerate(op(path, "rt")) if i > 0]
names = np.array([r[0] for r in rows])
s = np.array([r[2] for r in rows])
st = np.array([int(r[3]) for r in rows], dtype=np.float64)
en = np.array([int(r[4]) for r in rows], dtype=np.float64)
t0 = st.min()
st, en = (st - t0) / 1e6, (en - t0) / 1e6
is_spmm = np.char.find(names, "spmm") >= 0
main = collections.Counter(s[is_spmm]).most_common(1)[0][0]
m = s == main
o = np.argsort(st[m])
ms, me = st[m][o], en[m][o]
cuts = [0] + [i + 1 for i in range(len(ms) - 1) if ms[i + 1] - me[i] > 3.0] + [len(ms)]
print(f"main stream {main}: phases (start ms, end ms, kernels)")
for a, b in zip(cuts[:-1], cuts[1:]):
    print(f"   {ms[a]:8.1f} {me[b - 1]:8.1f} {b - a}")
A, B = ms[cuts[-2]], me[-1]
if len(sys.argv) > 3:
    A, B = float(sys.argv[2]), float(sys.argv[3])
print(f"timed region of the main stream: [{A:.1f}, {B:.1f}] ms = {B - A:.1f} ms")
for ss in [k for k, _ in collections.Counter(s).most_common(4)]:
    k = (s == ss) & (st >= A - 0.5)
    if not k.any():
        continue
    o = np.argsort(st[k])
    xs, xe = st[k][o], en[k][o]
    last, busy = xe[0], 0.0
    for i in range(len(xs)):
        if xs[i] - last > 1.5 and xs[i] > A + 50:
            break
        last = max(last, xe[i])
        busy += xe[i] - xs[i]
    print(f"stream {ss}: first start {xs[0]:.1f}, chain ends {last:.1f} ({last - A:.1f} ms after the region starts), kernel ms {busy:.1f}")
k = m & (st >= A - 0.5) & (en <= B + 0.5)
tot, cnt = collections.Counter(), collections.Counter()
for n, d in zip(names[k], (en - st)[k]):
    tot[n[:44]] += d
    cnt[n[:44]] += 1
nwin = max(1, int((k & is_spmm).sum()) // 13)   # 13 products per window
print(f"main stream kernels in the region: {sum(tot.values()):.1f} ms over {nwin} windows = {sum(tot.values()) / nwin:.2f} ms per window")
for n, v in tot.most_common(16):
    print(f"    {n:46s} {v:7.1f} ms  {cnt[n]:6d} calls  {1e3 * v / cnt[n]:8.1f} us avg  {v / nwin:6.2f} ms/window")
