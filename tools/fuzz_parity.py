"""Randomised parity sweep on the GPU: SWFD (device vs oracle/swfd_oracle.py) and kNN adjacency (device vs
oracle/mo_oracle.py) over random small shapes, batchings, dtypes and degenerate rows.  Prints one line per case and a
summary; exit code 1 on the first mismatch (the failing case is reproducible from its seed).

    python tools/fuzz_parity.py [--cases 60] [--seed 0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mused_amd import matrix_operations as mo
from mused_amd.swfd import SeqBasedSWFD as Dev
from oracle import mo_oracle as omo
from oracle.swfd_oracle import SeqBasedSWFD as Ora


def compare(dev, ora, tag):
    Bd, sd, ld, dd = dev.get()
    Bo, so, lo, do = ora.get()
    assert ld == lo, f"{tag}: level {ld} vs {lo}"
    s0 = max(so[0], 1e-300)
    if os.environ.get("FUZZ_VERBOSE"):
        print(tag, "\n dev sigma", sd, "\n ora sigma", so, "\n delta", dd, do, "level", ld, lo, flush=True)
    np.testing.assert_allclose(sd, so, rtol=0, atol=1e-8 * s0, err_msg=tag)
    np.testing.assert_allclose(Bd.T @ Bd, Bo.T @ Bo, rtol=0, atol=1e-8 * s0 * s0, err_msg=tag)
    assert abs(dd - do) <= 1e-8 * s0 * s0, tag


def swfd_case(rng, i):
    ell = int(rng.integers(2, 25))
    N = int(rng.integers(max(ell + 1, 8), 420))
    d = int(rng.integers(2, 90))
    kind = rng.choice(["gauss", "lowrank", "heavy", "binary", "zeros", "const"])
    n = int(rng.integers(N // 2, 3 * N + 50))
    if kind == "gauss":
        X = rng.standard_normal((n, d)) * rng.uniform(0.5, 20)
    elif kind == "lowrank":
        r = int(rng.integers(1, min(d, 6) + 1))
        X = rng.standard_normal((n, r)) @ rng.standard_normal((r, d)) + 1e-3 * rng.standard_normal((n, d))
    elif kind == "heavy":
        X = rng.standard_normal((n, d))
        X[rng.random(n) < 0.1] *= 40.0
    elif kind == "binary":
        X = (rng.random((n, d)) < 0.15).astype(np.int64)
    elif kind == "zeros":
        X = rng.standard_normal((n, d))
        X[rng.random(n) < 0.3] = 0.0
    else:
        X = np.tile(rng.standard_normal((1, d)), (n, 1))  # every row the same: rank one, exact duplicates
    Xf = X.astype(np.float64)
    R = max(float((Xf ** 2).sum(1).max()), 1.0) * float(rng.choice([1.0, 1.0, 3.7]))
    dev, ora = Dev(N=N, R=R, d=d, sketch_dim=ell), Ora(N=N, R=R, d=d, sketch_dim=ell)
    assert dev.L == ora.L
    t = 0
    checks = 0
    while t < n:
        step = int(rng.choice([1, 2, ell, ell + 1, N - 1, N, N + 1, int(rng.integers(1, 2 * N))]))
        step = max(1, min(step, n - t))
        blk = X[t:t + step]
        if rng.random() < 0.3:
            dev.fit(torch.from_numpy(np.ascontiguousarray(blk)).cuda())
        else:
            dev.fit(blk)
        ora.fit(blk)
        t += step
        if rng.random() < 0.5 or t == n:
            compare(dev, ora, f"swfd case {i} kind={kind} N={N} d={d} l={ell} t={t}")
            checks += 1
    dev.close()
    return f"swfd {kind:8s} N={N:3d} d={d:2d} l={ell:2d} rows={n:4d} L={ora.L} checks={checks}"


def knn_case(rng, i):
    n = int(rng.integers(2, 700))
    d = int(rng.integers(1, 48))
    kind = rng.choice(["gauss", "dups", "lattice", "zeros", "nonfinite"])
    X = rng.standard_normal((n, d))
    if kind == "dups":
        X[rng.integers(0, n, n // 3)] = X[rng.integers(0, n, n // 3)]
    elif kind == "lattice":
        X = rng.integers(-2, 3, size=(n, d)).astype(np.float64)
    elif kind == "zeros":
        X[rng.random(n) < 0.2] = 0.0
    elif kind == "nonfinite":
        X[rng.random(n) < 0.1, 0] = rng.choice([np.nan, np.inf, -np.inf])
    if rng.random() < 0.5:
        X = X.astype(np.float32)
    t = str(rng.choice(["", "cosine"]))
    nv = int(np.isfinite(X).all(axis=1).sum())
    k = int(rng.integers(0, max(nv, 1) + 1)) if rng.random() < 0.3 else int(rng.integers(0, min(nv, 60) + 1))
    try:
        ref = omo.create_adjacency_matrix(X.astype(np.float64), t, k)
        err = None
    except ValueError as e:
        ref, err = None, e
    if err is not None:
        try:
            mo.create_adjacency_matrix(X, t, k)
        except ValueError:
            return f"knn  {kind:9s} n={n:3d} d={d:2d} k={k:3d} type={t!r:8s} both raise"
        raise AssertionError(f"knn case {i}: oracle raised {err!r}, device did not")
    got = mo.create_adjacency_matrix(X, t, k)
    note = "ok"
    if not np.array_equal(got, ref):
        # Rows may differ only where the choice hangs on scores that are equal in exact arithmetic (duplicate rows,
        # lattice data): the host BLAS gives such pairs scores that differ in the last bits depending on which
        # micro-kernel handled the column (so does the reference), the device gives them equal scores and takes the
        # smaller row.  Everything that differs must sit within rounding of the row's k-th smallest score.
        valid = np.where(np.isfinite(X).all(axis=1))[0]
        Xv = X[valid].astype(np.float64)
        S = omo.cosine_scores(Xv) if t == "cosine" else omo.sq_euclidean_scores(Xv)
        kk = min(k + 1, len(valid)) if t == "cosine" else max(1, k)
        thr = np.partition(S, kk - 1, axis=1)[:, kk - 1][:, None]
        diff = (got != ref)[np.ix_(valid, valid)]
        scale = np.maximum(np.abs(thr), np.abs(S).max() * 1e-3)
        assert (np.abs(S - thr)[diff] <= 1e-12 * np.broadcast_to(scale, S.shape)[diff]).all(), \
            f"knn case {i} kind={kind} n={n} d={d} k={k} type={t!r} dtype={X.dtype}: {int(diff.sum())} entries differ beyond ties"
        # (degrees may differ by one in such rows: whether the row itself is among the tied picks decides if one of
        #  the k + 1 selected columns is dropped as the diagonal)
        note = f"equal up to {int(diff.sum())} tie entries"
    return f"knn  {kind:9s} n={n:3d} d={d:2d} k={k:3d} type={t!r:8s} dtype={X.dtype} {note}"


def lanes_case(rng, i):
    """B lock-step lanes (some of them fed IDENTICAL rows: the duplicate-skipping path) == B independent sketches bit
    for bit, and == the oracle within the SWFD tolerance."""
    ell = int(rng.integers(2, 20))
    N = int(rng.integers(max(ell + 1, 8), 300))
    d = int(rng.integers(2, 70))
    B = int(rng.integers(2, 7))
    n = int(rng.integers(N // 2, 2 * N + 40))
    dt = rng.choice([np.float32, np.float64])
    Xs = [rng.standard_normal((n, d)) * rng.uniform(0.5, 8) for _ in range(B)]
    for b in range(1, B):
        if rng.random() < 0.3:
            Xs[b] = Xs[int(rng.integers(0, b))]  # twin lanes
        elif rng.random() < 0.3:
            Xs[b] = (rng.random((n, d)) < 0.2).astype(np.float64)
    Xs = [x.astype(dt) for x in Xs]
    R = max(max(float((x.astype(np.float64) ** 2).sum(1).max()) for x in Xs), 1.0)
    lanes = Dev(N=N, R=R, d=d, sketch_dim=ell, lanes=B)
    singles = [Dev(N=N, R=R, d=d, sketch_dim=ell) for _ in range(B)]
    oras = [Ora(N=N, R=R, d=d, sketch_dim=ell) for _ in range(B)]
    X = torch.from_numpy(np.stack(Xs)).cuda()
    t = 0
    checks = 0
    while t < n:
        step = int(rng.choice([1, ell, ell + 1, N - 1, N, N + 1, int(rng.integers(1, 2 * N))]))
        step = max(1, min(step, n - t))
        lanes.fit_lanes(X[:, t:t + step])
        for b in range(B):
            singles[b].fit(X[b, t:t + step])
            oras[b].fit(Xs[b][t:t + step].astype(np.float64))
        t += step
        if rng.random() < 0.5 or t == n:
            Bl, sl, ll, dl = lanes.get()
            for b in range(B):
                Bs, ss, ls, ds = singles[b].get()
                tag = f"lanes case {i} N={N} d={d} l={ell} B={B} lane={b} t={t}"
                assert int(ll[b]) == ls and np.array_equal(Bl[b], Bs) and np.array_equal(sl[b], ss) and dl[b] == ds, tag
                compare(singles[b], oras[b], tag)
            checks += 1
    lanes.close()
    for sk in singles:
        sk.close()
    return f"lanes N={N:3d} d={d:2d} l={ell:2d} B={B} rows={n:3d} dtype={np.dtype(dt).name} checks={checks}"


def meta_case(rng, i):
    """Metadata modality types (matrix_operations.py:22-89) on random synthetic columns: device == oracle."""
    from mused_amd import synth

    n = int(rng.integers(2, 420))
    k = int(rng.integers(0, 40))
    cols, _ = synth.metadata_stream(n, int(rng.integers(0, 1 << 30)), events=int(rng.integers(1, 8)),
                                    users=int(rng.integers(3, 60)), vocab=int(rng.integers(8, 80)),
                                    missing=float(rng.choice([0.0, 0.05, 0.5, 1.0])), integer_time=bool(rng.random() < 0.5))
    if rng.random() < 0.3:  # duplicate geotags / stamps
        src = rng.integers(0, n, n // 2)
        dst = rng.integers(0, n, n // 2)
        cols["location"][dst] = cols["location"][src]
        cols["time"][dst] = cols["time"][src]
    out = []
    for t in ("location", "time", "username", "tags"):
        ref = omo.create_adjacency_matrix(cols[t], t, k)
        got = mo.create_adjacency_matrix(cols[t], t, k)
        if t == "location" and not np.array_equal(got, ref):
            # sin / cos / asin differ in the last bit between the device and the host libm: entries may move between
            # rows' selections only where two haversine distances agree to rounding
            valid, S, kk = omo.metadata_scores(cols[t], t, k)
            thr = np.partition(S, min(kk, len(valid)) - 1, axis=1)[:, min(kk, len(valid)) - 1][:, None]
            diff = (got != ref)[np.ix_(valid, valid)]
            assert (np.abs(S - thr)[diff] <= 1e-9 * np.maximum(thr, 1e-3).repeat(S.shape[1], 1)[diff]).all(), \
                f"meta case {i} location n={n} k={k}: differs beyond rounding of the haversine distance"
            out.append(f"location~{int(diff.sum())}")
            continue
        assert np.array_equal(got, ref), f"meta case {i} type={t} n={n} k={k}: {int((got != ref).sum())} entries differ"
        out.append(t)
    return f"meta n={n:3d} k={k:2d} " + " ".join(out)


def metawin_case(rng, i):
    """Random windows of a random metadata stream that was encoded once (mused_amd/meta.py, csrc/meta_window.hip) against
    the host path on the window's raw rows: bit for bit, whatever the share of invalid rows."""
    from mused_amd import meta, synth

    n = int(rng.integers(2, 900))
    k = int(rng.integers(0, 40))
    cols, _ = synth.metadata_stream(n, int(rng.integers(0, 1 << 30)), events=int(rng.integers(1, 8)),
                                    users=int(rng.integers(3, 60)), vocab=int(rng.integers(8, 80)),
                                    missing=float(rng.choice([0.0, 0.05, 0.5, 0.9])), integer_time=bool(rng.random() < 0.5))
    cols["tags"][rng.random(n) < rng.choice([0.0, 0.3]), 0] = ""   # rows the "tags" branch rejects
    if rng.random() < 0.3:  # duplicate geotags / stamps
        src, dst = rng.integers(0, n, n // 2), rng.integers(0, n, n // 2)
        cols["location"][dst] = cols["location"][src]
        cols["time"][dst] = cols["time"][src]
    windows = 0
    for t in ("location", "time", "username", "tags"):
        corpus = meta.encode(cols[t], t)
        for _ in range(4):
            s = int(rng.integers(0, n))
            e = int(rng.integers(s + 1, n + 1))
            got = mo.adjacency_on_device(corpus.window(s, e), t, k).to_numpy()
            ref = mo.adjacency_on_device(cols[t][s:e], t, k).to_numpy()
            assert np.array_equal(got, ref), f"metawin case {i} type={t} n={n} k={k} window=[{s}, {e}): " \
                                             f"{int((got != ref).sum())} entries differ"
            windows += 1
    return f"metawin n={n:3d} k={k:2d} windows={windows}"


def kmeans_ill_posed(emb, nc, seed, labels):
    """Adjudication of a label difference from the REFERENCE side: is the oracle's own k-means answer stable under a
    perturbation of its input at the level of one unit in the last place?  If scikit-learn's labels on `emb` change when
    `emb` is perturbed by 1e-15 of its largest entry (tied assignments: equal or zero embedding rows, equal singular
    values straddling the cut), the reference's answer is not a function of the window at the precision any fp64
    implementation -- including another LAPACK build -- can reproduce, and a difference is not a parity failure."""
    prng = np.random.default_rng(12345)
    scale = 1e-15 * max(float(np.abs(emb).max()), 1e-300)
    for _ in range(6):
        pert = emb + scale * prng.standard_normal(emb.shape)
        if not np.array_equal(omo.perform_clustering(pert, nc, seed), labels):
            return True
    return False


def cut_inside_multiple_sigma(sigma_all, n_comp):
    """The reference keeps the n_comp largest of the n_comp + 10 singular values its range finder resolves.  If the last kept
    and the first dropped one agree to 1e-9 of the largest, the kept subspace is an arbitrary slice of that eigenspace
    (picked by rounding inside LAPACK / the random projection): no fp64 implementation reproduces the reference's choice."""
    if sigma_all is None or len(sigma_all) <= n_comp:
        return False
    return abs(float(sigma_all[n_comp - 1]) - float(sigma_all[n_comp])) <= 1e-9 * float(sigma_all[0])


def rsvd_ill_posed(fused, ell, seed, nc, labels):
    """The same question one step earlier: are the REFERENCE's labels a function of the adjacency at the precision fp64
    can reproduce?  A multiple singular value that straddles the cut (seen: a 40-row graph with sigma = 1 fourteen-fold at
    l = 18) leaves the range finder an arbitrary subspace of that eigenspace, chosen by rounding: perturb the 0/1 matrix by
    1e-13 relative, run the oracle's whole eigenstep + k-means again, and call the case ill-posed if ITS labels move."""
    prng = np.random.default_rng(54321)
    A = np.asarray(fused, dtype=np.float64)
    for _ in range(4):
        pert = A * (1.0 + 1e-13 * prng.standard_normal(A.shape))
        emb_p, _, _ = omo.randomized_svd_reduce(pert, ell, seed)
        if not np.array_equal(omo.perform_clustering(emb_p, nc, seed), labels):
            return True
    return False


def rsvd_case(rng, i):
    """Eigenstep on a random kNN adjacency (one or two modalities OR-fused, some rows without any valid neighbour)."""
    n = int(rng.integers(24, 640))
    k = int(rng.integers(1, min(30, n - 1) + 1))
    M = int(rng.integers(1, 3))
    mods = []
    for _ in range(M):
        X = rng.standard_normal((n, int(rng.integers(2, 20))))
        if rng.random() < 0.4:
            X += 3.0 * rng.standard_normal((int(rng.integers(2, 6)), X.shape[1]))[rng.integers(0, 2, n)]
        if rng.random() < 0.3:
            X[rng.random(n) < 0.15, 0] = np.nan  # rows without edges (matrix_operations.py:114-115)
        mods.append(X)
    ell = int(rng.integers(1, min(40, n - 1) + 1))
    seed = int(rng.integers(0, 1000))
    adjs_o = [omo.create_adjacency_matrix(X, "", k) for X in mods]
    fused_o = omo.fuse_matrices(adjs_o)
    emb_o, sig_o, _ = omo.randomized_svd_reduce(fused_o, ell, seed)
    adjs_d = [mo.adjacency_on_device(X, "", k) for X in mods]
    fused_d = mo.fuse_matrices(adjs_d)
    assert np.array_equal(fused_d.to_numpy() != 0, fused_o != 0), f"rsvd case {i}: fused adjacency differs"
    emb_d, sig_d = mo.svd_reduce_on_device(fused_d, ell, seed)
    emb_d, sig_d = emb_d.cpu().numpy(), sig_d.cpu().numpy()
    s0 = sig_o[0]
    np.testing.assert_allclose(sig_d, sig_o, rtol=0, atol=1e-8 * s0, err_msg=f"rsvd case {i} n={n} k={k} l={ell} seed={seed}")
    # embedding columns: compared where the singular value is separated from its neighbours (a cluster of equal sigmas
    # may come out in any basis of its space)
    gaps = np.minimum(np.abs(np.diff(sig_o, prepend=np.inf)), np.abs(np.diff(sig_o, append=-np.inf)))
    clear = gaps > 2e-2 * s0  # (a near-complete graph has sigma_2 .. sigma_n within a few per cent of 1: seen at n = 30, k = 28)
    np.testing.assert_allclose(emb_d[:, clear], emb_o[:, clear], rtol=0, atol=1e-6 * np.abs(emb_o).max(),
                               err_msg=f"rsvd case {i} n={n} k={k} l={ell} seed={seed} (embedding)")
    nc = int(rng.integers(2, 7))
    lab_o = omo.perform_clustering(emb_o, nc, seed)
    lab_d = mo.perform_clustering(emb_d, nc, seed)
    same = np.array_equal(lab_o, lab_d)
    if not same:  # allowed only where the reference's own answer is ill-posed (see kmeans_ill_posed)
        assert kmeans_ill_posed(emb_o, nc, seed, lab_o) or rsvd_ill_posed(fused_o, ell, seed, nc, lab_o), (
            f"rsvd case {i} n={n} k={k} l={ell} seed={seed}: labels differ in {int((lab_o != lab_d).sum())} rows although the "
            "oracle's labels are stable under a 1e-15 perturbation of its embedding and a 1e-13 perturbation of its matrix")
    lab_dev = mo.perform_clustering_on_device(torch.from_numpy(emb_d).cuda(), nc, seed)
    assert np.array_equal(lab_dev, lab_d), f"rsvd case {i}: device k-means differs from scikit-learn on the same embedding"
    return f"rsvd n={n:3d} k={k:2d} M={M} l={ell:2d} seed={seed:3d} clear={int(clear.sum())}/{ell} labels {'equal' if same else 'differ in ' + str(int((lab_o != lab_d).sum())) + ' rows: ill-posed on the reference side (oracle labels move under a 1e-15 perturbation of its embedding or a 1e-13 perturbation of its matrix)'}"


def pipeline_case(rng, i):
    """Whole window loop against the oracle's restatement of main.py:13-130: random window size, hop ratio, modalities."""
    from mused_amd import synth
    from mused_amd.pipeline import process_streaming_data

    W = int(rng.integers(60, 260))
    ratio = int(rng.choice([1, 1, 2, 4]))
    while W % ratio:
        W += 1
    n = W * int(rng.integers(2, 5)) + int(rng.integers(0, W))
    ell = int(rng.integers(2, 12))
    k = int(rng.integers(3, 14))
    seed = int(rng.integers(0, 100))
    sseed = int(rng.integers(0, 10000))
    cols, labels = synth.metadata_stream(n, sseed, events=int(rng.integers(2, 6)))
    pool = {"": synth.blob_stream(n, int(rng.integers(2, 24)), sseed, n_centres=4)[0].astype(np.float64),
            "cosine": synth.blob_stream(n, int(rng.integers(3, 24)), sseed + 1, n_centres=4)[0].astype(np.float64),
            "location": cols["location"], "username": cols["username"], "text": synth.text_stream(n, sseed)[0]}
    types_ = [str(t) for t in rng.choice(list(pool), size=int(rng.integers(1, 4)), replace=False)]
    if types_ == ["username"]:
        # a same-user relation alone is a disjoint union of cliques: its singular values are the clique sizes - 1 with
        # multiplicities, a cluster of equal values straddles the cut at reduced_dim, and the retained directions --
        # hence the labels -- are then the arbitrary choice of the dense SVD routine (LAPACK's in the reference)
        types_.append("")
    mods = [pool[t] for t in types_]
    approach = str(rng.choice(["sSVDMC", "sSVDMC", "SWFDMC"]))
    if os.environ.get("FUZZ_VERBOSE"):
        print(f"pipeline case {i}: W={W} ratio={ratio} n={n} l={ell} k={k} seed={seed} types={types_} approach={approach}", flush=True)
    kw = {}
    if approach == "SWFDMC":
        from oracle.swfd_oracle import SeqBasedSWFD as OraSWFD
        kw["swfd_cls"] = OraSWFD
    otrace = []
    ref, ref_err = None, None
    try:
        ref = omo.process_streaming_data(mods, types_, W, ell, k, seed, approach, labels, step_window_ratio=ratio, trace=otrace, **kw)
    except ValueError as e:
        # scipy's linear_sum_assignment refuses a cost matrix that passes is_feasible (matrix_operations.py:226-233: no
        # all-inf row or column) but has no complete finite assignment; the reference lets that propagate (main.py:331)
        ref_err = e
    from mused_amd.pipeline import StreamPipeline

    got, got_err, dtrace = None, None, []
    pipe = StreamPipeline(W, ell, k, seed, approach, list(types_), ratio, async_labels=False)
    try:
        got = pipe.run(mods, np.asarray(labels))
    except ValueError as e:
        got_err = e
    finally:
        dtrace = list(pipe.trace)
        try:
            pipe.close()
        except ValueError:
            pass
    head = f"pipe W={W:3d} ratio={ratio} n={n:4d} l={ell:2d} k={k:2d} {approach:6s} types={types_}"
    if ref_err is not None and got_err is not None:
        assert str(got_err) == str(ref_err), f"pipeline case {i}: {got_err!r} vs {ref_err!r}"
        return f"{head} both raise {ref_err}"
    if ref_err is None and got_err is None and np.array_equal(np.asarray(got), np.asarray(ref)):
        return f"{head} labels equal ({len(ref)})"
    # The outcomes differ (labels, or one side raised).  Label chains are sequential: find the FIRST window whose raw
    # k-means labels differ and adjudicate it from the reference side -- a difference is accepted only if the oracle's own
    # k-means at that window is ill-posed (kmeans_ill_posed); everything after that window follows from it.
    first = None
    for w_, (do, dd) in enumerate(zip(otrace, dtrace)):
        if not np.array_equal(np.asarray(do["raw"]), np.asarray(dd["raw"])):
            first = w_
            break
    if first is None and len(dtrace) < len(otrace):
        first = len(dtrace)  # the device raised at this window (its trace records a window after the matching)
    assert first is not None, (f"pipeline case {i} {head}: outcomes differ (oracle: {ref_err!r}, device: {got_err!r}) although "
                               "every window's raw k-means labels agree")
    o = otrace[first]
    straddle = cut_inside_multiple_sigma(o.get("sigma_all"), len(o["sigma"])) if o.get("sigma") is not None else False
    assert straddle or kmeans_ill_posed(o["reduced"], o["n_clusters"], seed, o["raw"]), (
        f"pipeline case {i} {head}: raw labels differ at window {first} although the oracle's k-means there is stable under "
        "a 1e-15 perturbation of its input and its truncation does not cut through a multiple singular value")
    what = "labels differ" if (ref_err is None and got_err is None) else f"oracle: {ref_err!r}, device: {got_err!r}"
    why = "the reference's truncation cuts through a multiple singular value" if straddle else "oracle k-means ill-posed there (flips under a 1e-15 perturbation)"
    return f"{head} {what} from window {first} on: {why}"


CASES = {"swfd": swfd_case, "knn": knn_case, "rsvd": rsvd_case, "pipe": pipeline_case, "lanes": lanes_case, "meta": meta_case,
         "metawin": metawin_case}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=60)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", type=int, default=-1, help="run this case index only")
    ap.add_argument("--kinds", default="swfd,knn", help="comma-separated subset of swfd,knn,rsvd,pipe,lanes,meta,metawin (round robin)")
    a = ap.parse_args()
    t0 = time.time()
    np.set_printoptions(linewidth=200, precision=10)
    for i in (range(a.cases) if a.only < 0 else [a.only]):
        rng = np.random.default_rng([a.seed, i])
        kinds = a.kinds.split(",")
        fn = CASES[kinds[i % len(kinds)]]
        print(f"[{i:3d} seed=({a.seed},{i})]", fn(rng, i), f"({time.time() - t0:.0f}s)", flush=True)
    print(f"all {a.cases} cases passed")


if __name__ == "__main__":
    main()
