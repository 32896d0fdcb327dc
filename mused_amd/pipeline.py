"""Window loop of the streaming pipeline (the role of `process_streaming_data`, main.py:13-130),
built on the device engine.

Per full window (trigger rule of main.py:32):
    per-modality kNN adjacency (device bitmask)  ->  OR-fusion (or, with `modality_weights`, the weighted sum
    sum_m w_m A_m: the eigenstep then multiplies by a value per edge; the sketch approaches take bit rows and refuse it; or,
    with `fusion_threshold`, the 0/1 mask of the edges whose weighted agreement reaches the threshold, which every approach
    takes; `modality_ks`: a k per modality)  ->
        approach "sSVDMC"/"sSVDMC_hung"/"sSVDMC_pot"/"sSVDMC_mini": randomized-SVD embedding (main.py:79)
        approach "SWFDMC"             : SeqBasedSWFD over the rows of the fused matrix, R from the
                                        first window only, sketch transposed to (W, l)  (main.py:58-76)
    -> k-means with n_clusters = #distinct true labels in the window (main.py:41,97); "sSVDMC_mini": one MiniBatchKMeans
       (n_clusters_total) for the whole stream, partial_fit + predict per window IN WINDOW ORDER (main.py:82-86)
       "DBSCAN_incr": one IncrementalDBSCAN(eps, min_samples) for the whole stream, insert + get_cluster_labels per window IN
       WINDOW ORDER (main.py:87-91; mused_amd/incdbscan.py, csrc/dbscan_incr.hip: the labels of a DBSCAN refit on every row
       inserted so far; with `dbscan_max_rows` over a sliding window of that many rows: the oldest rows are deleted on the
       device before each insert, and the labels are those of a refit on the rows still held)
    -> Hungarian matching against the previous window, min_overlap = 3 (main.py:110); "sSVDMC_pot": matching by the
       Sinkhorn transport plan (main.py:111) in csrc/match.hip
    -> labels appended (main.py:118-119).

Device work of window t+1 is enqueued while the host runs k-means / matching of window t
(`async_labels=True`): the embedding is copied to pinned memory behind an event, a worker thread
waits on the event and runs the scikit-learn / SciPy consumers in window order.
"""
from __future__ import annotations

import os
import threading
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import matrix_operations as mo
from . import meta as _meta
from . import text as _text
from ._lib import MusedError
from . import fusion as _fusion
from .engine import MAX_WEIGHTED_PARTS, WindowEngine, check_threshold, check_weights
from .swfd import SeqBasedSWFD


def check_ks(modality_ks, count=None):
    """`modality_ks` as a list of ints, one k per modality, every one >= 1 (ValueError otherwise); None stays None."""
    if modality_ks is None:
        return None
    try:
        ks = list(modality_ks)
    except TypeError:
        raise ValueError(f"modality_ks must be a sequence of integers, got {modality_ks!r}") from None
    for x in ks:
        if isinstance(x, (bool, float, str)) or not isinstance(x, (int, np.integer)) or x < 1:
            raise ValueError(f"modality_ks must be integers >= 1, got {x!r}")
    if count is not None and len(ks) != count:
        raise ValueError(f"{len(ks)} modality ks for {count} modalities")
    return [int(x) for x in ks]


def check_k_range(n_clusters_range, approach, n):
    """`n_clusters_range` as (lo, hi) with 2 <= lo <= hi <= n - 1, or None.  ValueError for anything else, for the approaches
    that take no k per window ("sSVDMC_mini": one clusterer for the stream; "DBSCAN_incr", "DBSCAN_batch", "HDBSCAN_batch":
    no k at all) and under MUSED_KMEANS=host (the selector has no host form)."""
    import numbers

    if n_clusters_range is None:
        return None
    if approach in ("sSVDMC_mini", "DBSCAN_incr", "DBSCAN_batch", "HDBSCAN_batch"):
        raise ValueError(f"n_clusters_range: approach {approach!r} takes no k per window")
    if os.environ.get("MUSED_KMEANS", "device") == "host":
        raise ValueError("n_clusters_range: the selector runs on the device only (MUSED_KMEANS=host is set)")
    try:
        lo, hi = n_clusters_range
    except (TypeError, ValueError):
        raise ValueError(f"n_clusters_range must be (lo, hi), got {n_clusters_range!r}") from None
    for v in (lo, hi):
        if not isinstance(v, numbers.Integral) or isinstance(v, bool):
            raise ValueError(f"n_clusters_range must hold two ints, got {n_clusters_range!r}")
    if not 2 <= lo <= hi <= n - 1:
        raise ValueError(f"n_clusters_range = {n_clusters_range!r}: need 2 <= lo <= hi <= rows - 1 = {n - 1}")
    return int(lo), int(hi)


def check_vote(fusion_threshold, modality_weights, count=None):
    """The arguments of a fusion by agreement threshold as (tau, vote weights or None); with the number of modalities known
    also checked against it (more than 8 modalities, a threshold above the sum of all weights: ValueError)."""
    w = None if modality_weights is None else check_weights(modality_weights, count)
    if w is None and count is not None:
        if not 1 <= count <= MAX_WEIGHTED_PARTS:
            raise ValueError(f"a threshold fusion takes 1 .. {MAX_WEIGHTED_PARTS} modalities, got {count}")
        w = [1.0] * count
    if w is not None:
        return check_threshold(w, fusion_threshold)[1], (None if modality_weights is None else w)
    tau = float(fusion_threshold)
    if not (np.isfinite(tau) and tau > 0.0):
        raise ValueError(f"the fusion threshold must be finite and > 0, got {fusion_threshold!r}")
    return tau, None


class StreamPipeline:
    def __init__(self, window_size, reduced_dim, k_basis, seed, approach="sSVDMC", modality_types=None,
                 step_window_ratio=1, engine=None, async_labels=True, feature_sketch=False, stream=None,
                 assume_finite=False, window_slots=1, n_clusters_total=None, eps=0.5, min_samples=5,
                 dbscan_max_rows=None, modality_weights=None, fusion_threshold=None, modality_ks=None,
                 n_clusters_range=None, internal_scores=False, align_embeddings=False):
        if approach not in ("sSVDMC", "sSVDMC_hung", "sSVDMC_pot", "sSVDMC_mini", "SWFDMC", "DBSCAN_incr"):
            raise ValueError(f"approach {approach!r} is not on the device hot path")
        # `align_embeddings` (off by default: nothing below runs then).  The two chained approaches feed every window's
        # embedding into ONE stream-long clusterer, but each window's coordinates are its own singular vectors.  With the
        # option window 0 defines the frame and window t is carried onto the ALIGNED window t - 1 by the orthogonal
        # Procrustes map of the rows the two share (matrix_operations.align_embedding_on_device) -- an isometry of the whole
        # window, applied on the chain worker immediately before the clusterer takes the embedding.  Per window:
        # `alignment_residuals` = |A R - B| / |B| and `alignment_unaligned` = |A - B| / |B| over the shared rows, NaN for window 0.
        self._align = bool(align_embeddings)
        if self._align:
            if approach not in ("sSVDMC_mini", "DBSCAN_incr"):
                raise ValueError(f"align_embeddings: approach {approach!r} clusters every window on its own -- k-means is invariant "
                                 "under the map, and a sketch is no eigenstep embedding; it serves 'sSVDMC_mini' and 'DBSCAN_incr'")
            if int(step_window_ratio) <= 1:
                raise ValueError("align_embeddings: with step_window_ratio = 1 consecutive windows share no rows to align on")
            if int(window_slots) > 1:
                raise ValueError("align_embeddings: the alignment is a chain over windows in order; window_slots must be 1")
        self.alignment_residuals, self.alignment_unaligned = [], []
        self._align_ref = None    # (the previous window's aligned embedding, the stream row of its first row)
        # WITHOUT GROUND TRUTH (both off by default: nothing below runs then).  `n_clusters_range` = (lo, hi): every k-means
        # window chooses its own k among lo .. hi by the device silhouette (matrix_operations.select_n_clusters_on_device)
        # instead of taking the number of distinct true labels, which may then be None; the k of every window: `chosen_k`.
        # `internal_scores`: silhouette, Davies-Bouldin and Calinski-Harabasz of every window's (embedding, raw labels), on
        # the label worker's stream before the matching: `internal_scores`, a list of dicts in window order (NaNs for a
        # window whose labels hold a single value).
        self._k_range = check_k_range(n_clusters_range, approach, int(window_size))
        self._internal = bool(internal_scores)
        self.chosen_k, self.internal_scores = [], []
        # None: OR-fusion, today's path exactly.  M weights (finite, > 0): the modalities are fused by weighted sum and the
        # eigenstep runs valued.  The sketches ingest bit rows: weighted rows for them are not built
        # `fusion_threshold` (tau): the fused matrix is the 0/1 mask of the edges whose weighted agreement
        # sum_m w_m [A_m has the edge] reaches tau (mused_amd/fusion.py; weights 1.0 without `modality_weights`, which then only
        # weight the vote).  A 0/1 matrix again: every approach takes it, the sketches included, on the binary eigenstep
        self.weights = None
        self.threshold = self.vote_weights = self._table = None
        n_mods = len(modality_types) if modality_types else None
        if fusion_threshold is not None:
            self.threshold, self.vote_weights = check_vote(fusion_threshold, modality_weights, n_mods)
        elif modality_weights is not None:
            if approach == "SWFDMC" or feature_sketch:
                raise ValueError("modality_weights: the SWFD sketch ingests the bit rows of the OR-fused adjacency; weighted "
                                 "fusion covers the approaches that go through the eigenstep")
            self.weights = check_weights(modality_weights, len(modality_types) if modality_types else None)
        if approach == "sSVDMC_mini" and n_clusters_total is None:
            raise ValueError("approach 'sSVDMC_mini' needs n_clusters_total (MiniBatchKMeans(n_clusters=n_clusters_total), "
                             "main.py:84)")
        # "sSVDMC_mini": ONE clusterer for the stream (mused_amd.cluster.MiniBatchKMeans, built at the first window on the
        # thread that clusters).  Its state is a chain over windows, so its clustering runs on the chain worker, in window
        # order, not in the parallel k-means pool; the device work of later windows (slots included) still overlaps it.
        self._mini = approach == "sSVDMC_mini"
        # "DBSCAN_incr": embedding as "sSVDMC"; ONE mused_amd.incdbscan.IncrementalDBSCAN(eps, min_samples) for the stream takes
        # every window's embedding in window order -- a chain like the one above, on the chain worker, with one window slot
        self._incr = approach == "DBSCAN_incr"
        self._chained = self._mini or self._incr
        # eps="auto" ("DBSCAN_incr"): the stream's IncrementalDBSCAN chooses eps from the first window's embedding
        # (matrix_operations.select_eps_on_device) and keeps it: `chosen_eps` once that window has been clustered
        if isinstance(eps, str) and eps != "auto":
            raise ValueError(f'eps must be a number or "auto", got {eps!r}')
        self.eps, self.min_samples = eps, min_samples
        # None: the state only grows (main.py:87-91).  A number: IncrementalDBSCAN(max_rows=...), at least one window
        self.dbscan_max_rows = None if dbscan_max_rows is None else int(dbscan_max_rows)
        if self.dbscan_max_rows is not None and self.dbscan_max_rows < int(window_size):
            raise ValueError(f"dbscan_max_rows = {dbscan_max_rows} is smaller than a window ({window_size} rows)")
        # "sSVDMC_pot": embedding and k-means as "sSVDMC"; the label chain matches by the Sinkhorn plan (main.py:111), every
        # other approach by SciPy's assignment (main.py:110).  Both chains run on the device (csrc/match.hip,
        # csrc/match_hung.hip), or on the host (mused_amd/sinkhorn.py, SciPy) under MUSED_MATCH=host
        self._pot = approach == "sSVDMC_pot"
        self._match_device = os.environ.get("MUSED_MATCH", "device") != "host"
        self.n_clusters_total = None if n_clusters_total is None else int(n_clusters_total)
        self.clusterer = None
        self.W, self.ell, self.k, self.seed = int(window_size), int(reduced_dim), int(k_basis), int(seed)
        # a k per modality: modality m uses ks[m] wherever the reference uses k_basis for it ("time" still takes 3 k + 1 ...)
        self.ks = check_ks(modality_ks, n_mods)
        self.approach = approach
        self.types = modality_types
        # rows with a non-finite entry are dropped from the kNN (matrix_operations.py:114-115).  Finding out needs one
        # small host read per window (on a side stream, so it does not wait for the previous window's device work);
        # `assume_finite=True` skips it for callers that generate their rows (the benchmark's synthetic stream)
        self.assume_finite = bool(assume_finite)
        self._chk = None
        self.ratio = step_window_ratio
        self.eng = engine or WindowEngine(self.W)
        # WINDOW SLOTS (sSVDMC only): adjacency -> fusion -> eigenstep of one window is a chain of ~1,600 small dependent
        # launches that leaves most of the GPU idle (25 ms of latency, a few per cent of its throughput); windows are
        # independent until the label chain, so consecutive windows go to `window_slots` engines on their own streams
        # (each driven by its own host thread: launching the 1,600-node graph costs ~20 ms of host time) and overlap.
        # Measured at config 2 (Cholesky-QR eigenstep): 9.9 -> 6.6 ms per window with 4 slots (1.01 M -> 1.5 M rows/s);
        # 2 slots can be slower than one, the best count varies with how HIP maps the streams onto hardware queues.
        # Opt-in (default 1; MUSED_WINDOW_SLOTS for
        # process_streaming_data).  The sketch approaches carry state from window to window and keep one slot.
        self._nslots = max(1, int(window_slots)) if (approach not in ("SWFDMC", "DBSCAN_incr") and not feature_sketch) else 1
        # Every engine records its eigenstep graph once, on the caller's thread, before the slot threads exist (see
        # process_window).  A modality without an edge bound ("username") re-creates an engine's handle -- frees, graph
        # destruction, allocations, a new capture -- whenever a window has more edges than the handle was sized for; the
        # library serialises those resource calls with every capture of the process (csrc/internal.h: capture_mutex;
        # round 2 ran them beside another slot's capture and aborted, gpurun_out/r2_gputest23.log).  Such streams still
        # keep one slot: a re-creation stalls every slot behind that lock for tens of milliseconds.
        if self._optimistic_nnz():
            self._nslots = 1
        # DEFERRED FLAGS: the candidate-list overflow of the fused kNN and the weak-pivot / edge-count flags of the
        # eigenstep are not read on the enqueueing thread; they travel to the host behind the window's event and a
        # flagged (rare) window is repeated by the label worker on a fallback engine (classic kNN path, the reference's
        # LU / Householder chain).  Not for the sketch approaches: the adjacency feeds a sketch that cannot be rewound.
        self._defer = approach != "SWFDMC" and os.environ.get("MUSED_DEFER_FLAGS", "1") != "0"
        self._fb_eng = None
        self._fb_lock = threading.Lock()
        self.redone_windows = 0
        self._nnz_hint = 0         # edges of the densest window seen so far ("username": no a-priori bound)
        self._closed = False
        # reuse across hopping windows (one engine, every window in order).  Default: from ratio 4 on -- measured at config 2
        # (W = 10^4, d = 1024, tools/hop_reuse_time.py): similarity + selection per window 2.70 ms from scratch, with reuse
        # 2.90 ms at ratio 2 (the phases that establish the entering rows' thresholds run on too few tiles to fill the GPU),
        # 2.19 ms at ratio 4, 1.96 ms at ratio 8.  MUSED_HOP_REUSE=1 / 0 forces it on (any ratio > 1) / off.
        hr = os.environ.get("MUSED_HOP_REUSE")
        self._hop_reuse = self._nslots == 1 and int(step_window_ratio) > 1 and (
            hr == "1" or (hr != "0" and int(step_window_ratio) >= 4))
        self._slots = None        # [(engine, stream)], built at the first window
        self._nwin = 0
        self.swfd = None          # SWFDMC sketch over fused-adjacency rows (d = W)
        self.feature_sketch = feature_sketch
        self.fswfd = None         # optional SWFD over the raw feature rows (BASELINE config 2 wording)
        self.prev = None
        self.out = []
        self.trace = []
        self.latencies = []
        # host consumers: k-means of different windows is independent (a small pool), the Hungarian matching is a
        # chain over windows (one worker, jobs run in submission order)
        nk = max(1, int(os.environ.get("MUSED_LABEL_WORKERS", "3")))
        self._kpool = ThreadPoolExecutor(max_workers=nk) if async_labels else None
        self._pool = ThreadPoolExecutor(max_workers=1) if async_labels else None
        self._max_inflight = nk + 2
        self.host_ms = {"kmeans": [], "match": []}
        # scikit-learn's k-means takes one OpenMP thread per visible core; on a many-core host (256 on the MI355X
        # boxes) that is ~3x slower for a (10k, 128) problem than a handful of threads
        self._omp_limit = None
        self._blas_limit = None
        try:
            from threadpoolctl import threadpool_limits

            want = int(os.environ.get("MUSED_LABEL_THREADS", "8"))
            if want > 0 and (os.cpu_count() or 1) > want:
                self._omp_limit = threadpool_limits(limits=want, user_api="openmp")
            # k-means calls BLAS from inside its OpenMP loops and caps it at one thread around them -- by flipping
            # the process-wide BLAS pool size, which several k-means workers do concurrently and out of step
            # (OpenBLAS then warns "Detect OpenMP Loop and this application may hang"): pin it at one thread here
            self._blas_limit = threadpool_limits(limits=1, user_api="blas") if nk > 1 and async_labels else None
        except Exception:  # threadpoolctl missing: keep the library default
            self._omp_limit = None
        # k-means of the embedding: k-means++ seeding and Lloyd iterations on the device unless
        # MUSED_KMEANS=host; MUSED_KMEANS_SEED=host keeps scikit-learn's seeding on the host.  Every label worker drives
        # its own high-priority stream.  (Windows that fell back: matrix_operations.km_fallbacks.)
        self._km_device = os.environ.get("MUSED_KMEANS", "device") != "host"
        self._km_seed_device = self._km_device and os.environ.get("MUSED_KMEANS_SEED", "device") != "host"
        self._km_local = threading.local()
        self.km_device_windows = 0
        self._pending = deque()
        # the feature-row sketch is independent of the adjacency / eigenstep of the same window: it
        # runs on its own HIP stream and the two meet again before the results are handed to the host
        # (only when this pipeline has the GPU to itself: HIP maps streams onto a handful of hardware
        # queues -- 4 by default -- and streams sharing a queue run in order, so concurrent pipelines
        # use ONE stream each and overlap with each other instead)
        self._side = torch.cuda.Stream(priority=-1) if (feature_sketch and stream is None) else None
        # all device work of this pipeline is enqueued on `stream` (default: the current stream), so
        # several pipelines -- each owning a contiguous block of windows -- can share one GPU
        self._stream = stream
        # pinned staging buffers are recycled: allocating pinned memory synchronises the device, which
        # would serialise concurrent pipelines
        self._pins = []
        self._flag_pins = []
        self._pin_lock = threading.Lock()
        self._dpools = None
        self._device = torch.cuda.current_device()  # worker threads must select it themselves

    # ---- device side of one window --------------------------------------------------------------
    def window_device(self, mods, eng=None, defer=False, lo=None):
        """mods: list of (W, d_m) float32/float64 tensors on the device.  Returns (reduced (W, m) CUDA
        tensor, sigma CUDA tensor, flags): flags = None (sketch approaches), the eigenstep's int32[4] flag word, or with
        `defer` the int32[12] word of `WindowEngine.window_flags` (nothing read on this thread)."""
        eng = eng or self.eng
        eng.begin_window(defer)
        try:
            return self._window_device(mods, eng, defer, lo)
        finally:
            eng.defer = False  # direct callers of the engine get finished results again

    def _window_device(self, mods, eng, defer, lo=None):
        types = self.types or [""] * len(mods)
        # hopping windows (step_window_ratio > 1): consecutive windows share rows -> the dense modalities reuse their
        # candidate lists across windows (engine.knn_adjacency_hop).  `lo` = stream row of the window's row 0.
        reuse = lo is not None and self._hop_reuse and eng is self.eng
        ks = self._ks(len(mods))
        adjs = [self._adjacency(m, t, eng, hop=((i, lo) if reuse else None), k=ks[i]) for i, (m, t) in enumerate(zip(mods, types))]
        if self.threshold is not None:
            fused = self._fuse_vote(adjs, eng)              # a subset of the OR mask: every edge bound below holds
        elif self.weights is not None:
            if len(self.weights) != len(adjs):
                raise ValueError(f"{len(self.weights)} modality weights for {len(adjs)} modalities")
            fused = eng.fuse_weighted(adjs, self.weights)   # the pattern is the OR mask: every edge bound below holds
        else:
            fused = eng.fuse(adjs) if len(adjs) > 1 else adjs[0]
            if len(adjs) == 1:
                fused.fused = False
        if self.feature_sketch:
            X = mods[0] if len(mods) == 1 else torch.cat(mods, dim=1)
            if self.fswfd is None:
                R = float((X.double() ** 2).sum(dim=1).max().item())
                self.fswfd = SeqBasedSWFD(N=self.W, R=R, d=X.shape[1], sketch_dim=self.ell)
            if self._side is not None:
                main = torch.cuda.current_stream()
                self._side.wait_stream(main)
                with torch.cuda.stream(self._side):
                    X.record_stream(self._side)
                    self.fswfd.fit(X)
                    self.feature_B, self.feature_sigma, _ = self.fswfd.get_device()
            else:
                self.fswfd.fit(X)
                self.feature_B, self.feature_sigma, _ = self.fswfd.get_device()
        if self.approach == "SWFDMC":
            if self.swfd is None:  # main.py:60-62
                R = self.eng.max_row_sq_norm(fused)
                self.swfd = SeqBasedSWFD(N=self.W, R=R, d=fused.n, sketch_dim=self.ell)
            self.swfd.fit_adjacency(fused)  # rows of the fused 0/1 matrix straight from the bitmask (no W x W dense)
            B, sigma, _ = self.swfd.get_device()
            reduced = B.t().contiguous() if B.shape[0] != self.W else B  # main.py:73-76
            return reduced, sigma, None
        # edges per row: k selected (l2; the row itself is normally one of them) or k + 1 (cosine / text)
        per_row = [mo.edges_per_row(t, k) for t, k in zip(types, ks)]
        if all(b is not None for b in per_row):
            nnz_cap = fused.n * sum(per_row)
        elif defer:
            # "username": as many edges as a user has rows.  Optimistic bound (the densest window so far, 8 per row to
            # begin with); a window with more raises flags[0] and is repeated with its exact count by the label worker
            nnz_cap = max(self._nnz_hint, fused.n * (8 + sum(b or 0 for b in per_row)))
        else:  # count them (blocking)
            nnz_cap = max(int(fused.degrees()[2][1].item()), 1)
            self._nnz_hint = max(self._nnz_hint, nnz_cap + nnz_cap // 4)
        emb, sigma, flags = eng.svd_reduce(fused, self.ell, self.seed, nnz_cap=nnz_cap, want_flags=True)
        if defer:
            flags = eng.window_flags(flags)
        return emb, sigma, flags

    def _ks(self, n_mods):
        """k of each of the window's modalities: `modality_ks`, or k_basis for all."""
        if self.ks is None:
            return [self.k] * n_mods
        if len(self.ks) != n_mods:
            raise ValueError(f"{len(self.ks)} modality ks for {n_mods} modalities")
        return self.ks

    def _fuse_vote(self, adjs, eng=None):
        """The thresholded 0/1 mask of one window's modality adjacencies (the table is built at the first window)."""
        if self._table is None:
            tau, w = check_vote(self.threshold, self.vote_weights, len(adjs))
            self._table = _fusion.threshold_table(w if w is not None else [1.0] * len(adjs), tau)
        return (eng or self.eng).fuse_table(adjs, self._table)

    def _fuse_binary(self, adjs, eng=None):
        """The 0/1 matrix the sketches ingest: the thresholded mask, or the OR mask."""
        if self.threshold is not None:
            return self._fuse_vote(adjs, eng)
        return (eng or self.eng).fuse(adjs) if len(adjs) > 1 else adjs[0]

    def _adjacency(self, m, t, eng=None, hop=None, k=None):
        """One modality of one window -> device adjacency, with the reference's row filtering.  k: this modality's k (k_basis
        without it)."""
        eng = eng or self.eng
        k = self.k if k is None else k
        if t == "text" or t in mo._METADATA_TYPES or not isinstance(m, torch.Tensor):
            # (text: thousands of documents tie at similarity 0 and overflow the candidate lists in most windows -- the
            # overflow word is read at once there instead of repeating the whole window, TF-IDF included, afterwards)
            was, eng.defer = eng.defer, eng.defer and t != "text"
            try:
                return mo.adjacency_on_device(m, t, k, engine=eng)
            finally:
                eng.defer = was
        metric = mo._metric_for(t)
        if not self.assume_finite and m.is_floating_point():
            if self._chk is None:
                with self._pin_lock:  # slot threads may get here together
                    if self._chk is None:
                        self._chk = torch.cuda.Stream()
            # The check runs on a side stream so that it does not wait for the previous window's device work -- but it
            # must see the rows: the side stream waits for an event recorded on the stream this window is enqueued on
            # (which already waits for whatever produced the rows on the caller's stream, _device_side), nothing more
            ev = torch.cuda.Event()
            ev.record()
            self._chk.wait_event(ev)
            m.record_stream(self._chk)
            with torch.cuda.stream(self._chk):
                ok = bool(torch.isfinite(m).all().item())
            if not ok:
                return mo.adjacency_on_device(m, t, k, engine=eng)
        if hop is not None:
            return eng.knn_adjacency_hop(m, k, metric, key=hop[0], lo=hop[1])
        return eng.knn_adjacency(m, k, metric)

    # ---- host consumers -------------------------------------------------------------------------
    def _cluster(self, job):
        """Independent per window: wait for the embedding, k-means (main.py:97)."""
        ev, red_pin, sig_pin, n_clusters, trigger, t_start = job[:6]
        flag_pin, reduced_dev, mods = job[6], job[7], job[8]
        slot_keys, job_eng = (job[9], job[10]) if len(job) > 10 else ([], self.eng)
        torch.cuda.set_device(self._device)
        ev.synchronize()
        on_dev = self._rows_stay_on_device(reduced_dev)
        reduced_host, sigma_host = None if on_dev else red_pin.numpy().copy(), sig_pin.numpy().copy()
        flags_host = flag_pin.numpy().copy() if flag_pin is not None else None
        with self._pin_lock:
            self._pins.append((red_pin, sig_pin))
            if flag_pin is not None:
                self._flag_pins.append(flag_pin)
        if flags_host is not None:
            redo = len(flags_host) > 4 and (flags_host[2] != 0 or flags_host[4:].any()
                                            or (flags_host[0] != 0 and self._optimistic_nnz()))
            if redo:
                # a candidate list overflowed / the final Cholesky-QR met a weak pivot / more edges than the optimistic
                # bound: this window again, on the paths that have no such limits (rare; blocking on this worker only)
                for i_, f_ in enumerate(flags_host[4:]):   # hopping-window reuse: rebuild that modality's state next window
                    key = slot_keys[i_] if i_ < len(slot_keys) else None   # (flag word i_ <-> the i_-th DEFERRED kNN call)
                    if f_ and key is not None:
                        job_eng.request_hop_reset(key)
                reduced_dev, sigma_dev, flags_host = self._redo_window(mods)
                reduced_host, sigma_host = reduced_dev.cpu().numpy(), sigma_dev.cpu().numpy()
            WindowEngine.check_rsvd_flags(flags_host)  # raised on the label worker, surfaces in flush()
        t0 = time.perf_counter()
        if self._align:
            reduced_dev, reduced_host = self._aligned(reduced_dev, reduced_host, job[11] if len(job) > 11 else None)
        if self._mini:
            clusters = self._minibatch(reduced_dev, reduced_host)
        elif self._incr:
            clusters = self._dbscan_incr(reduced_dev, reduced_host)
        elif self._km_device and reduced_dev is not None and reduced_dev.dtype == torch.float64:
            st = getattr(self._km_local, "stream", None)
            if st is None:
                st = self._km_local.stream = torch.cuda.Stream(priority=-1)
            reduced_dev.record_stream(st)  # produced on the pipeline's stream, complete (ev), consumed on the worker's
            if self._k_range is not None:
                n_clusters, clusters, _ = mo.select_n_clusters_on_device(
                    reduced_dev, range(self._k_range[0], self._k_range[1] + 1), self.seed, stream=st, emb_host=reduced_host)
            else:
                clusters = mo.perform_clustering_on_device(reduced_dev, n_clusters, self.seed, emb_host=reduced_host, stream=st)
            self.km_device_windows += 1
        elif self._k_range is not None:
            raise ValueError("n_clusters_range: the window's embedding is not an fp64 device tensor; the selector has no host form")
        else:
            clusters = mo.perform_clustering(reduced_host, n_clusters, self.seed)
        self.host_ms["kmeans"].append(1e3 * (time.perf_counter() - t0))
        if self._k_range is not None or self._internal:
            return clusters, sigma_host, n_clusters, self._internal_scores(reduced_dev, clusters) if self._internal else None
        return clusters, sigma_host

    def _internal_scores(self, reduced_dev, clusters):
        """The three truth-free indices of (embedding, raw labels) on this label worker's stream; the embedding is read where
        it lies on the device.  Labels with a single value have no such score: NaNs."""
        from . import metrics_evaluation as me

        if reduced_dev is None:
            raise ValueError("internal_scores: the window's embedding is not on the device")
        st = getattr(self._km_local, "stream", None)
        if st is None:
            st = self._km_local.stream = torch.cuda.Stream(priority=-1)
        reduced_dev.record_stream(st)  # produced on the pipeline's stream, complete (ev), consumed on the worker's
        flags, n_labels, s, db, ch, Xd = me.internal_metrics_raw(reduced_dev, np.asarray(clusters), st, wait_current=False)
        if flags & 2:
            me._raise_flags(flags, n_labels, Xd)
        return {"silhouette": s, "davies_bouldin": db, "calinski_harabasz": ch}

    def _rows_stay_on_device(self, reduced):
        """A k-means window with device seeding: nothing on the host reads the embedding (the labels, sigma and the flag
        words are all the trace and the matching take), so it is not copied to the pinned buffer; a window that falls back
        fetches it itself (matrix_operations._km_host_copy)."""
        return self._km_seed_device and not self._chained and reduced is not None and reduced.dtype == torch.float64

    def _aligned(self, reduced_dev, reduced_host, lo):
        """align_embeddings: this window's embedding in the frame of window 0 -> (device tensor, host array), one of them None:
        the form the clusterer takes (the device tensor unless MUSED_KMEANS=host hands 'sSVDMC_mini' the host copy).  Called in
        window order on the chain worker, on its stream; `lo` = stream row of the window's first row."""
        if lo is None:
            raise ValueError("align_embeddings needs the stream row of every window (process_window(..., lo=...))")
        on_dev = reduced_dev is not None and reduced_dev.dtype == torch.float64 and (self._incr or self._km_device)
        cur = reduced_dev if on_dev else np.ascontiguousarray(reduced_host, dtype=np.float64)
        res = un = float("nan")
        if self._align_ref is not None:
            ref, ref_lo = self._align_ref
            shift = int(lo) - int(ref_lo)
            if not 0 < shift < self.W:
                raise ValueError(f"align_embeddings: windows at stream rows {ref_lo} and {lo} share no rows")
            if on_dev:
                st = getattr(self._km_local, "stream", None)
                if st is None:
                    st = self._km_local.stream = torch.cuda.Stream(priority=-1)
                reduced_dev.record_stream(st)  # produced on the pipeline's stream, complete (ev), consumed on the worker's
                cur, _, res, un = mo.align_embedding_on_device(reduced_dev, ref, shift, stream=st)
            else:
                cur, _, res, un = mo._align_scipy(cur, ref, shift)
        self._align_ref = (cur, lo)
        self.alignment_residuals.append(res)
        self.alignment_unaligned.append(un)
        return (cur, None) if on_dev else (None, cur)

    def _minibatch(self, reduced_dev, reduced_host):
        """main.py:82-86: clusterer.partial_fit(reduced).predict(reduced) on the stream's one MiniBatchKMeans.  Called in
        window order (chain worker, or the caller without async labels).  labels_ after partial_fit IS predict on the same
        rows: the same E step on the same centres (compute_labels=True)."""
        if not self._km_device:   # MUSED_KMEANS=host: scikit-learn's own class
            if self.clusterer is None:
                from sklearn.cluster import MiniBatchKMeans as SkMiniBatchKMeans

                self.clusterer = SkMiniBatchKMeans(n_clusters=self.n_clusters_total, random_state=self.seed, batch_size=self.W)
            return self.clusterer.partial_fit(reduced_host).predict(reduced_host)
        from .cluster import MiniBatchKMeans

        st = getattr(self._km_local, "stream", None)
        if st is None:
            st = self._km_local.stream = torch.cuda.Stream(priority=-1)
        if self.clusterer is None:
            self.clusterer = MiniBatchKMeans(n_clusters=self.n_clusters_total, random_state=self.seed, batch_size=self.W,
                                             stream=st)
        if reduced_dev is not None and reduced_dev.dtype == torch.float64:
            reduced_dev.record_stream(st)  # produced on the pipeline's stream, complete (ev), consumed on the worker's
            X = reduced_dev
        else:
            X = np.ascontiguousarray(reduced_host, dtype=np.float64)
        self.km_device_windows += 1
        return self.clusterer.partial_fit(X).labels_

    @property
    def chosen_eps(self):
        """The eps the stream's IncrementalDBSCAN runs with ("DBSCAN_incr"; None before its first window and for the other
        approaches): the number given, or the one eps="auto" chose."""
        return getattr(self.clusterer, "eps_", None) if self._incr else None

    def _dbscan_incr(self, reduced_dev, reduced_host):
        """main.py:87-91: clusterer.insert(reduced).get_cluster_labels(reduced) on the stream's one IncrementalDBSCAN.  Called
        in window order (chain worker, or the caller without async labels)."""
        from .incdbscan import IncrementalDBSCAN

        st = getattr(self._km_local, "stream", None)
        if st is None:
            st = self._km_local.stream = torch.cuda.Stream(priority=-1)
        if self.clusterer is None:
            self.clusterer = IncrementalDBSCAN(eps=self.eps, min_pts=self.min_samples, stream=st, max_rows=self.dbscan_max_rows)
        if reduced_dev is not None and reduced_dev.dtype == torch.float64:
            reduced_dev.record_stream(st)  # produced on the pipeline's stream, complete (ev), consumed on the worker's
            X = reduced_dev
        else:
            X = np.ascontiguousarray(reduced_host, dtype=np.float64)
        return self.clusterer.insert(X).get_cluster_labels(X)

    def _cluster_chain(self, job):
        """sSVDMC_mini, DBSCAN_incr: the clustering and the matching of one window, both on the chain worker (window order)."""
        self._chain(self._cluster(job), job)

    def _optimistic_nnz(self):
        return any(mo.edges_per_row(t, self.k) is None for t in (self.types or []))   # ("username": whatever its k)

    def _redo_window(self, mods):
        """One window on the fallback engine (score-matrix kNN, LU / Householder eigenstep, exact edge count), on the
        calling worker's stream; returns (reduced, sigma, host flags)."""
        with self._fb_lock:
            if self._fb_eng is None:
                self._fb_eng = WindowEngine(self.W)
                self._fb_eng.knn_mode = "classic"
                self._fb_eng.rsvd_mode = "lu"
            st = getattr(self._km_local, "stream", None)
            if st is None:
                st = self._km_local.stream = torch.cuda.Stream(priority=-1)
            with torch.cuda.stream(st):
                for m in mods:
                    if isinstance(m, torch.Tensor):
                        m.record_stream(st)
                reduced, sigma, flags = self.window_device(mods, self._fb_eng, defer=False)
                flags_host = flags.cpu().numpy()
                st.synchronize()
            self.redone_windows += 1
            if self.redone_windows == 8 or (self.redone_windows > 8 and self.redone_windows % 64 == 0):
                import warnings

                warnings.warn(f"mused_amd: {self.redone_windows} windows of this stream were repeated on the fallback engine "
                              "(candidate-list overflow / weak pivot / edge bound): correct, but several times slower", RuntimeWarning)
            return reduced, sigma, flags_host

    def _chain(self, fut, job):
        """Sequential over windows: matching against the previous window (main.py:105-119), Hungarian or, for
        "sSVDMC_pot", by the Sinkhorn plan."""
        res = fut.result() if hasattr(fut, "result") else fut
        clusters, sigma_host = res[0], res[1]
        if len(res) > 2:   # n_clusters_range / internal_scores: kept in window order, like everything this worker appends
            if self._k_range is not None:
                self.chosen_k.append(int(res[2]))
            if self._internal:
                self.internal_scores.append(res[3])
        trigger, t_start = job[4], job[5]
        t0 = time.perf_counter()
        method = "pot" if self._pot else "hungarian"
        if self._match_device:
            torch.cuda.set_device(self._device)
            st = getattr(self._km_local, "stream", None)
            if st is None:
                st = self._km_local.stream = torch.cuda.Stream(priority=-1)
            # Hungarian approaches: what the narrow chain cannot take (a label outside [0, 1024), more than 256 labels a side)
            # goes to csrc/match_wide.hip, not to the host.  DBSCAN_incr's windows hold the noise label -1, which the narrow
            # chain would only flag: straight to the wide one.  MUSED_MATCH_WIDE=host (read per call): the former host route
            wide = False if self._pot else ("only" if self._incr else True)
            matched = mo.match_clusters_on_device(self.prev, clusters, min_overlap=3, stream=st, method=method, wide=wide)
        else:
            matched = mo.match_clusters(self.prev, clusters, method=method, min_overlap=3)
        if matched is None or len(matched) == 0:  # main.py:114-116
            matched = np.full(self.W, 0)
        self.host_ms["match"].append(1e3 * (time.perf_counter() - t0))
        self.prev = matched
        self.out.extend(matched)
        self.trace.append(dict(trigger=trigger, sigma=sigma_host, raw=np.asarray(clusters), matched=np.asarray(matched)))
        self.latencies.append(time.perf_counter() - t_start)

    def _get_pins(self, reduced, sigma):
        while True:
            with self._pin_lock:
                for i, (rp, sp) in enumerate(self._pins):
                    if rp.shape == reduced.shape and sp.shape == sigma.shape:
                        return self._pins.pop(i)
            if self._nslots == 1 and len(self._pending) >= self._max_inflight:  # back-pressure: reuse a buffer
                self._pending.popleft().result()
                continue
            return (torch.empty(reduced.shape, dtype=reduced.dtype, pin_memory=True),
                    torch.empty(sigma.shape, dtype=sigma.dtype, pin_memory=True))

    def _device_side(self, mods, n_clusters, trigger, t_start, eng, st, wait_ev, lo=None):
        """Enqueue one window on (eng, st); returns the job the label workers consume."""
        torch.cuda.set_device(self._device)
        if wait_ev is not None:
            st.wait_event(wait_ev)  # whatever produced the rows on the caller's stream
        with torch.cuda.stream(st):
            if self._nslots > 1:
                for m in mods:
                    if isinstance(m, torch.Tensor):
                        m.record_stream(st)
            reduced, sigma, flags = self.window_device(mods, eng, defer=self._defer, lo=lo)
            if self._side is not None:
                torch.cuda.current_stream().wait_stream(self._side)  # window latency includes the sketch
            red_pin, sig_pin = self._get_pins(reduced, sigma)
            if not self._rows_stay_on_device(reduced):
                red_pin.copy_(reduced, non_blocking=True)
            sig_pin.copy_(sigma, non_blocking=True)
            flag_pin = None
            if flags is not None:
                with self._pin_lock:
                    flag_pin = self._flag_pins.pop() if self._flag_pins else None
                if flag_pin is None or flag_pin.numel() != flags.numel():
                    flag_pin = torch.empty(flags.numel(), dtype=torch.int32, pin_memory=True)
                flag_pin.copy_(flags, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        # (slot -> hop-state key of this window's deferred flag words: the engine has moved on by the time a worker reads them)
        return (ev, red_pin, sig_pin, n_clusters, trigger, t_start, flag_pin, reduced, mods, list(eng.slot_keys), eng, lo)

    def _submit(self, job):
        """Hand a window to the label workers (async mode)."""
        if self._chained:
            return self._pool.submit(self._cluster_chain, job)
        return self._pool.submit(self._chain, self._kpool.submit(self._cluster, job), job)

    def _cluster_chain_after(self, fut_job):
        return self._cluster_chain(fut_job.result())

    def _cluster_after(self, fut_job):
        return self._cluster(fut_job.result())

    def _chain_after(self, fut_cluster, fut_job):
        return self._chain(fut_cluster, fut_job.result())

    def process_window(self, mods, true_labels_window, trigger=None, lo=None):
        """One full window.  `lo`: stream row of its first row -- given for hopping windows it lets the dense modalities
        reuse the previous window's similarity work (only with one engine and windows handed in in order)."""
        t_start = time.perf_counter()
        # main.py:41 (with n_clusters_range the window chooses its k itself and the true labels may be None)
        n_clusters = len(np.unique(true_labels_window)) if self._k_range is None else None
        caller = torch.cuda.current_stream()
        if self._slots is None:
            first = self._stream if self._stream is not None else caller
            if self._nslots == 1:
                self._slots = [(self.eng, self._stream)]  # stream None: whatever is current at each call
            else:
                # every slot on a stream of its own (none of them the caller's: a slot then waits for the caller's stream --
                # whatever produced the rows -- without waiting for another slot's window) and with a host thread of its
                # own: launching the ~1,600-node eigenstep graph costs ~20 ms of host time per window
                self._slots = [(self.eng if i == 0 else WindowEngine(self.W), torch.cuda.Stream(priority=first.priority))
                               for i in range(self._nslots)]
                self._dpools = [ThreadPoolExecutor(max_workers=1) for _ in range(self._nslots)]
                # Every engine records its eigenstep graph at its first window.  Do that here, one engine after the other
                # and before any worker thread exists.  What a ThreadLocal capture does not survive on this runtime is a
                # DEVICE-WIDE synchronisation made by another host thread while it records (tools/repro_capture_threads.hip:
                # hipDeviceSynchronize beside a capture fails 38 of 40 captures with "operation failed due to a previous
                # error during capture"; allocations, frees, launches, graph / stream creation and destruction, stream and
                # event synchronisation beside it: 0 of 40) -- the library therefore serialises its captures with its own
                # handle creation / destruction (capture_mutex) and nothing here calls torch.cuda.synchronize() off the
                # caller's thread.
                for e_, s_ in self._slots:
                    s_.wait_stream(caller)
                    with torch.cuda.stream(s_):
                        self.window_device(mods, e_, defer=self._defer)
                    s_.synchronize()
        slot = self._nwin % self._nslots
        eng, st = self._slots[slot]
        st = st if st is not None else caller
        self._nwin += 1
        if self._nslots == 1 or self._pool is None:
            if self._nslots > 1:
                st.wait_stream(caller)
            job = self._device_side(mods, n_clusters, trigger, t_start, eng, st, None, lo)
            if self._pool is None:
                self._chain(self._cluster(job), job)
            else:
                self._pending.append(self._submit(job))
            return
        while len(self._pending) >= self._max_inflight + self._nslots:  # back-pressure (pinned buffers, engines)
            self._pending.popleft().result()
        wait_ev = torch.cuda.Event()
        wait_ev.record(caller)
        fut_job = self._dpools[slot].submit(self._device_side, mods, n_clusters, trigger, t_start, eng, st, wait_ev)
        if self._chained:
            self._pending.append(self._pool.submit(self._cluster_chain_after, fut_job))
            return
        fut_cluster = self._kpool.submit(self._cluster_after, fut_job)
        self._pending.append(self._pool.submit(self._chain_after, fut_cluster, fut_job))

    def process_reduced(self, reduced: torch.Tensor, sigma: torch.Tensor, true_labels_window, trigger=None):
        """Hand the label workers a window whose reduced matrix (W, m) is already on the device (current stream): k-means
        (main.py:97) and the trace entry {trigger, sigma, raw, matched}.  For drivers that produce the embedding themselves
        (`SwfdmcLanes`); the matching of `out` follows the order of the calls, `trace[i]["raw"]` is order independent."""
        t_start = time.perf_counter()
        n_clusters = len(np.unique(true_labels_window)) if self._k_range is None else None
        red_pin, sig_pin = self._get_pins(reduced, sigma)
        if not self._rows_stay_on_device(reduced):
            red_pin.copy_(reduced, non_blocking=True)
        sig_pin.copy_(sigma, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        job = (ev, red_pin, sig_pin, n_clusters, trigger, t_start, None, reduced, None, [], self.eng)
        if self._pool is None:
            self._chain(self._cluster(job), job)
        else:
            self._pending.append(self._submit(job))

    def flush(self):
        """Wait for every window handed in so far; re-raises the first error a worker met (the remaining windows are
        still drained, so that nothing is in flight afterwards)."""
        first = None
        while self._pending:
            try:
                self._pending.popleft().result()
            except BaseException as e:  # noqa: BLE001 -- re-raised below
                first = first or e
        if first is None:
            for s in (self.swfd, self.fswfd):
                if s is not None:
                    s.check()  # an eigensolve of the sketch that gave up invalidates its results
        if first is not None:
            raise first

    def run(self, data_modalities, true_labels):
        """Stream whole modalities (host or device arrays) through the window loop; returns the
        concatenated event labels (`all_clusters`, main.py:125)."""
        dev = []
        types = self.types or [""] * len(data_modalities)
        for m, t in zip(data_modalities, types):
            if isinstance(m, (_text.TextCorpus, _meta.MetaCorpus)):
                dev.append(m)
                continue
            if t in mo._METADATA_TYPES and mo.meta_on_device():
                # encoded once for the whole stream (validity, user ids, tag sets and their posting lists); every window
                # is a view of the corpus and one launch on its resident arrays (MUSED_META=host: the rows stay as they
                # are and every window is handled on the host)
                c = _meta.encode(m, t)
                if not c.host_only:
                    c.device_arrays(self.eng.device)
                dev.append(c)
                continue
            if isinstance(m, torch.Tensor):
                dev.append(m.cuda())
                continue
            if t == "text" and mo.text_on_device():
                # tokenised once for the whole stream; every window is a view of the corpus and its TF-IDF runs on the
                # device (MUSED_TEXT=host: the strings stay as they are and every window is vectorised on the host)
                # (MUSED_TOKENISE=device|host: which tokeniser, `text.tokenise_for_device`)
                dev.append(_text.tokenise_for_device(m, self.eng.device))
                continue
            a = np.asarray(m)
            # numeric modalities live on the device; other string records stay on the host
            dev.append(torch.from_numpy(np.ascontiguousarray(a)).cuda() if a.dtype.kind in "fiub" else a)
        torch.cuda.current_stream().synchronize()  # rows resident before the first window (see _adjacency)
        n = dev[0].shape[0]
        for i in range(n):
            if i + 1 >= self.W and (i + 1) * self.ratio % self.W == 0:  # main.py:32
                lo = i + 1 - self.W
                self.process_window([m[lo : i + 1] for m in dev], None if true_labels is None else true_labels[lo : i + 1], trigger=i,
                                    lo=lo if self.ratio > 1 else None)
        self.flush()
        return np.array(self.out)

    def close(self):
        """Deterministic teardown, also after a failed flush(): workers are drained and joined first, then the device is
        idle, then every handle this pipeline created is destroyed -- nothing is left to `__del__` / interpreter exit."""
        if self._closed:
            return
        self._closed = True
        err = None
        try:
            self.flush()
        except BaseException as e:  # noqa: BLE001 -- re-raised after the teardown
            err = e
        for dp in (self._dpools or []):
            dp.shutdown(wait=True)
        self._dpools = None
        if self._pool is not None:
            self._kpool.shutdown(wait=True)
            self._pool.shutdown(wait=True)
        try:  # the streams this pipeline enqueued on (no device-wide synchronisation: another pipeline may be capturing)
            for _, st in (self._slots or []):
                if st is not None:
                    st.synchronize()
            for st in (self._stream, self._side, self._chk):
                if st is not None:
                    st.synchronize()
            torch.cuda.current_stream().synchronize()
        except Exception as e:  # noqa: BLE001
            err = err or e
        for s in (self.swfd, self.fswfd):
            if s is not None:
                s.close()
        self.swfd = self.fswfd = None
        for e, _ in (self._slots or [])[1:]:
            e.close()
        self._slots = None
        if self._fb_eng is not None:
            self._fb_eng.close()
            self._fb_eng = None
        for lim in (self._blas_limit, self._omp_limit):
            if lim is not None:
                lim.restore_original_limits()
        self._blas_limit = self._omp_limit = None
        if err is not None:
            raise err

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:  # the body failed: tear down, keep the body's exception
            try:
                self.close()
            except BaseException:  # noqa: BLE001
                pass
        return False


def process_streaming_data(results, data_modalities, modality_types, window_size, reduced_dim, k_basis, n_clusters_total,
                           seed, approach, complete_true_labels, step_window_ratio, noise_rate, label_mode, sorting,
                           eps, min_samples, score=False, modality_weights=None, fusion_threshold=None, modality_ks=None,
                           n_clusters_range=None, internal_scores=False, partition_scores=False, align_embeddings=False):
    """Same positional parameters as main.py:13.  `modality_weights` (one weight per modality, finite and > 0): fusion by
    weighted sum instead of OR for the approaches that go through the eigenstep ("SWFDMC": ValueError); None: OR.
    `fusion_threshold` (tau): every window's fused matrix is the 0/1 mask of the edges whose agreement sum_m w_m [modality m
    has the edge] is >= tau -- for every approach, "SWFDMC" and "DBSCAN_incr" included; `modality_weights` then only weight
    the vote (1.0 each without them).  `modality_ks`: one k >= 1 per modality, used wherever the reference uses k_basis for
    that modality; k_basis is what the scored results report.  Returns `results` with the label arrays ("all_clusters") and the wall
    time ("processing_time").  `score=True`: `results` (get_initial_results()'s lists when none is given) also receives
    what the reference's compute_all_metrics appends (main.py:128: the concatenated window labels against the
    concatenated true labels of main.py:39-40, which repeat rows when step_window_ratio > 1; "processing_time" is then
    the reference's list), and "window_scores", the (K, 7) scores of the K windows from one launch
    (metrics_evaluation.score_windows).
    `eps="auto"` ("DBSCAN_incr"; the other approaches ignore eps as before): the stream's IncrementalDBSCAN chooses eps from
    the first window's embedding (matrix_operations.select_eps_on_device, k = min_samples) and keeps it:
    `results["chosen_eps"]`.
    `n_clusters_range` = (lo, hi): every window chooses its k among lo .. hi by the device silhouette instead of taking it from
    the true labels (`results["chosen_k"]`, one per window; `complete_true_labels` may then be None unless `score`); ValueError
    for "sSVDMC_mini" and "DBSCAN_incr" and under MUSED_KMEANS=host.  `internal_scores=True`: `results["internal_scores"]`, per
    window the dict of metrics_evaluation.compute_internal_metrics on (embedding, raw labels), NaNs where the labels hold a
    single value.  `partition_scores=True`: `results["partition_scores"]`, the dict of
    metrics_evaluation.compute_partition_metrics (ARI, AMI, V-measure, ..., matched accuracy: scores that ignore how clusters
    are numbered) on the same concatenated labels, and `results["window_partition_scores"]`, the (K, 9) array of
    metrics_evaluation.partition_windows; ValueError when `complete_true_labels` is None.
    `align_embeddings=True` ("sSVDMC_mini" and "DBSCAN_incr" with step_window_ratio > 1; ValueError otherwise): every window's
    embedding is carried into the frame of window 0 by the orthogonal Procrustes map of the rows it shares with the window
    before it, ahead of the stream's clusterer; `results["alignment_residuals"]` and `results["alignment_unaligned"]`, one
    entry per window, NaN for the first."""
    if score and complete_true_labels is None:
        raise ValueError("score=True compares against complete_true_labels, which is None")
    if partition_scores and complete_true_labels is None:
        raise ValueError("partition_scores=True compares against complete_true_labels, which is None")
    # MUSED_DBSCAN_INCR_ROWS (read at every call; DBSCAN_incr only): the rows the stream's IncrementalDBSCAN holds at most
    incr_rows = os.environ.get("MUSED_DBSCAN_INCR_ROWS") if approach == "DBSCAN_incr" else None
    t0 = time.time_ns()
    # modality types go through unchanged: "" / anything the reference does not special-case = Euclidean kNN
    # (matrix_operations.py:112), "text" and "cosine" = the cosine kernel, the other SED2012 metadata types raise
    with StreamPipeline(window_size, reduced_dim, k_basis, seed, approach, list(modality_types), step_window_ratio,
                        window_slots=int(os.environ.get("MUSED_WINDOW_SLOTS", "1")), n_clusters_total=n_clusters_total,
                        eps=eps, min_samples=min_samples, dbscan_max_rows=int(incr_rows) if incr_rows else None,
                        modality_weights=modality_weights, fusion_threshold=fusion_threshold, modality_ks=modality_ks,
                        n_clusters_range=n_clusters_range, internal_scores=internal_scores,
                        align_embeddings=align_embeddings) as pipe:
        clusters = pipe.run(data_modalities, None if complete_true_labels is None else np.asarray(complete_true_labels))
    t1 = time.time_ns()
    if score:
        results = _scored(results, clusters, _window_true_labels(complete_true_labels, len(data_modalities[0]), window_size,
                                                                 step_window_ratio),
                          (len(data_modalities[0]), noise_rate, label_mode, sorting, reduced_dim, k_basis, window_size), t1, t0,
                          window_size)
    else:
        results = dict(results or {})
        results["all_clusters"] = clusters
        results["processing_time"] = (t1 - t0) / 1e9
    if approach == "DBSCAN_incr" and isinstance(eps, str):
        results["chosen_eps"] = pipe.chosen_eps
    if n_clusters_range is not None:
        results["chosen_k"] = list(pipe.chosen_k)
    if internal_scores:
        results["internal_scores"] = list(pipe.internal_scores)
    if align_embeddings:
        results["alignment_residuals"] = list(pipe.alignment_residuals)
        results["alignment_unaligned"] = list(pipe.alignment_unaligned)
    if partition_scores:
        _partition_scored(results, clusters, _window_true_labels(complete_true_labels, len(data_modalities[0]), window_size,
                                                                 step_window_ratio), window_size)
    return results


def _window_true_labels(complete_true_labels, n, window_size, step_window_ratio):
    """all_true_labels of main.py:39-40: the true labels of every processed window, concatenated."""
    labels = np.asarray(complete_true_labels)
    parts = [labels[i + 1 - window_size : i + 1] for i in range(n)
             if i + 1 >= window_size and (i + 1) * step_window_ratio % window_size == 0]   # main.py:32
    return np.concatenate(parts) if parts else labels[:0]


def _scored(results, clusters, true_labels, variables, t1, t0, window_size=None):
    """`results` after the reference's compute_all_metrics call (main.py:128, :165), plus "all_clusters" and, for a
    stream, the per-window scores."""
    from . import metrics_evaluation as me

    results = dict(results) if results else me.get_initial_results()[0]
    clusters = np.asarray(clusters)
    me.compute_all_metrics(results, *variables, clusters, true_labels, t1, t0)
    results["all_clusters"] = clusters
    if window_size is not None:
        results["window_scores"] = (me.score_windows(true_labels.reshape(-1, window_size), clusters.reshape(-1, window_size))
                                    if len(clusters) else np.empty((0, 7)))
    return results


def _partition_scored(results, clusters, true_labels, window_size=None):
    """Adds "partition_scores" (and, for a stream, "window_partition_scores") to `results`."""
    from . import metrics_evaluation as me

    clusters, true_labels = np.asarray(clusters), np.asarray(true_labels)
    results["partition_scores"] = me.compute_partition_metrics(true_labels, clusters)
    if window_size is not None:
        results["window_partition_scores"] = (me.partition_windows(true_labels.reshape(-1, window_size),
                                                                   clusters.reshape(-1, window_size))
                                              if len(clusters) else np.empty((0, len(me.PARTITION_KEYS))))


BATCH_APPROACHES = ("SVDMC_batch", "DBSCAN_batch", "HDBSCAN_batch")


def batch_embedding(data_modalities, modality_types, reduced_dim, k_basis, seed, engine=None, timings=None,
                    modality_weights=None, fusion_threshold=None, modality_ks=None):
    """Device part of process_batch_data (main.py:138-147): per-modality kNN adjacency of all rows, OR-fused into one
    bitmask as it arrives (one modality mask alive beside the fused one), then the randomized-SVD embedding at n = subset
    size.  Returns (embedding (n, m) fp64 CUDA tensor, sigma, number of fused edges).  `timings`: a dict that receives
    the seconds of every phase (synchronised) and, as "peak_bytes", the most device memory in use beyond what was in
    use on entry at the end of any phase.  `modality_weights`: fusion by weighted sum (every modality's mask then stays alive
    until the eigenstep has read it, and the eigenstep holds 16 bytes of values per edge).  `fusion_threshold`: fusion by
    agreement threshold (process_streaming_data); the vote needs every modality's bit at once, so the masks cannot be ORed as
    they arrive: every modality's mask stays alive until the one fusion launch, as on the weighted path (M + 1 masks at the
    peak instead of 2); the eigenstep is the binary one.  `modality_ks`: one k per modality instead of k_basis."""
    n = len(data_modalities[0])
    threshold = None
    if fusion_threshold is not None:
        threshold, weights = check_vote(fusion_threshold, modality_weights, len(data_modalities))
    else:
        weights = None if modality_weights is None else check_weights(modality_weights, len(data_modalities))
    ks = check_ks(modality_ks, len(data_modalities)) or [k_basis] * len(data_modalities)
    parts = []
    base = torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0] if timings is not None else 0
    eng = engine or WindowEngine(max(n, 2))

    def tick(name, t):
        if timings is not None:
            torch.cuda.synchronize()
            timings[name] = timings.get(name, 0.0) + time.perf_counter() - t
            free, total = torch.cuda.mem_get_info()  # device memory in use beyond what was in use on entry
            timings["peak_bytes"] = max(timings.get("peak_bytes", 0), total - free - base)
        return time.perf_counter()

    try:
        fused = None
        t = time.perf_counter()
        for i, (m, ty) in enumerate(zip(data_modalities, modality_types)):
            if len(m) != n:
                raise ValueError(f"modality {i} has {len(m)} rows, modality 0 has {n}")
            if ty == "text" and mo.text_on_device() and not isinstance(m, (_text.TextCorpus, _text.TextWindow)):
                m = _text.tokenise_for_device(m, eng.device)   # the whole subset is one window of this corpus
                t = tick(f"tokenise[{i}]", t)
            adj = mo.adjacency_on_device(m, ty, ks[i], engine=eng)
            t = tick(f"knn[{i}:{ty or 'l2'}]", t)
            if weights is not None or threshold is not None:
                parts.append(adj)
            else:
                fused = adj if fused is None else eng.fuse_into(fused, adj)
            del adj
            t = tick("fusion", t)
        if threshold is not None:
            fused = eng.fuse_threshold(parts, threshold, weights)
            parts.clear()
        elif weights is not None:
            fused = eng.fuse_weighted(parts, weights)
        deg, _, _ = fused.degrees()
        nnz = int(deg.to(torch.int64).sum().item())
        if nnz >= 2 ** 31:
            raise MusedError(f"the fused adjacency has {nnz} edges: the eigenstep's neighbour lists are int32 (< 2^31)")
        t = tick("fusion", t)
        emb, sig, flags = eng.svd_reduce(fused, reduced_dim, seed, nnz_cap=max(nnz, 1), want_flags=True)
        WindowEngine.check_rsvd_flags(flags.cpu().numpy())
        tick("eigenstep", t)
        return emb, sig, nnz
    finally:
        if engine is None:
            eng.close()


def process_batch_data(results, data_modalities, modality_types, reduced_dim, k_basis, n_clusters, seed, approach,
                       complete_true_labels, noise_rate, label_mode, sorting, eps, min_samples, min_cluster_size,
                       window_size, timings=None, score=False, modality_weights=None, fusion_threshold=None, modality_ks=None,
                       n_clusters_range=None, internal_scores=False, partition_scores=False):
    """`modality_weights`, `fusion_threshold`, `modality_ks`: as for process_streaming_data (every batch approach goes through
    the eigenstep; see batch_embedding for what a threshold costs in memory).  `n_clusters_range`, `internal_scores`: as for
    process_streaming_data with the subset as the one window ("SVDMC_batch" chooses its k; the density approaches raise).
    Same positional parameters as main.py:132: the whole subset as one window -- kNN adjacency per modality, fusion,
    randomized-SVD embedding on the device (`batch_embedding`), then "SVDMC_batch": k-means with n_clusters on the device
    (perform_clustering_on_device: scikit-learn's labels); "DBSCAN_batch": DBSCAN on the device embedding
    (perform_dbscan_clustering_on_device: scikit-learn's labels, csrc/dbscan.hip); "HDBSCAN_batch": MUSED_HDBSCAN, read at every call --
    unset or `package`: the host wrapper around the `hdbscan` package on the embedding, as the reference does; `device`:
    perform_hdbscan_clustering_on_device on the device embedding (scikit-learn's HDBSCAN labels, csrc/emst.hip; pinned to
    scikit-learn, NOT to the package, hence opt-in); `sklearn`: scikit-learn's estimator on a host copy.  Returns `results` with the labels ("all_clusters") and the wall time
    ("processing_time"), like process_streaming_data.  `timings`: see batch_embedding (plus "clustering" and "edges").
    `score=True`: `results` also receives what the reference's compute_all_metrics appends (main.py:165).
    `eps="auto"` ("DBSCAN_batch"): eps is chosen from the embedding by matrix_operations.select_eps_on_device (k = min_samples)
    and stored as `results["chosen_eps"]`.
    `partition_scores=True`: `results["partition_scores"]`, as for process_streaming_data."""
    if approach not in BATCH_APPROACHES:
        raise ValueError(f"approach {approach!r} is not a batch approach {BATCH_APPROACHES}")
    hd_mode = os.environ.get("MUSED_HDBSCAN", "package") if approach == "HDBSCAN_batch" else None
    if hd_mode is not None and hd_mode not in ("package", "device", "sklearn"):
        raise ValueError(f"MUSED_HDBSCAN={hd_mode!r}: expected package, device or sklearn")
    if hd_mode == "package":
        import hdbscan  # noqa: F401  (the reference imports it at module level: without it nothing runs)
    k_range = check_k_range(n_clusters_range, approach, len(data_modalities[0]))
    if score and complete_true_labels is None:
        raise ValueError("score=True compares against complete_true_labels, which is None")
    if partition_scores and complete_true_labels is None:
        raise ValueError("partition_scores=True compares against complete_true_labels, which is None")
    t0 = time.time_ns()
    emb, _, nnz = batch_embedding(data_modalities, list(modality_types), reduced_dim, k_basis, seed, timings=timings,
                                  modality_weights=modality_weights, fusion_threshold=fusion_threshold, modality_ks=modality_ks)
    t1 = time.perf_counter()
    if hd_mode == "device":
        clusters = mo.perform_hdbscan_clustering_on_device(emb, min_cluster_size=min_cluster_size, min_samples=min_samples)
    elif hd_mode == "sklearn":
        clusters = mo.perform_hdbscan_clustering_sklearn(emb.cpu().numpy(), min_cluster_size=min_cluster_size,
                                                         min_samples=min_samples)
    elif hd_mode == "package":
        clusters = mo.perform_hdbscan_clustering(emb.cpu().numpy(), min_cluster_size=min_cluster_size,
                                                 min_samples=min_samples)
    elif approach == "DBSCAN_batch":
        chosen_eps = None
        if isinstance(eps, str):   # "auto": chosen from the embedding (matrix_operations.select_eps_on_device)
            if eps != "auto":
                raise ValueError(f'eps must be a number or "auto", got {eps!r}')
            eps = chosen_eps = mo.select_eps_on_device(emb, min_samples)[0]
        clusters = mo.perform_dbscan_clustering_on_device(emb, eps=eps, min_samples=min_samples)
    elif k_range is not None:
        n_clusters, clusters, _ = mo.select_n_clusters_on_device(emb, range(k_range[0], k_range[1] + 1), seed)
    else:
        clusters = mo.perform_clustering_on_device(emb, n_clusters, seed)
    scores = None
    if internal_scores:
        from . import metrics_evaluation as me

        flags, n_labels, s, db, ch, Xd = me.internal_metrics_raw(emb, np.asarray(clusters))
        if flags & 2:
            me._raise_flags(flags, n_labels, Xd)
        scores = {"silhouette": s, "davies_bouldin": db, "calinski_harabasz": ch}   # NaNs: the labels hold a single value
    if timings is not None:
        timings["clustering"] = time.perf_counter() - t1
        timings["edges"] = nnz
    t_end = time.time_ns()
    if score:
        results = _scored(results, clusters, np.array(complete_true_labels),
                          (len(data_modalities[0]), noise_rate, label_mode, sorting, reduced_dim, k_basis, window_size), t_end, t0)
    else:
        results = dict(results or {})
        results["all_clusters"] = np.asarray(clusters)
        results["processing_time"] = (t_end - t0) / 1e9
    if approach == "DBSCAN_batch" and chosen_eps is not None:
        results["chosen_eps"] = chosen_eps
    if k_range is not None:
        results["chosen_k"] = [int(n_clusters)]
    if scores is not None:
        results["internal_scores"] = [scores]
    if partition_scores:
        _partition_scored(results, clusters, np.array(complete_true_labels))
    return results


class SwfdmcLanes:
    """The reference's SWFDMC approach (main.py:58-76: one SeqBasedSWFD over the rows of the fused W x W adjacency of every
    window, d = W; get() transposed to (W, l) -> k-means -> matching) with the windows of a stream dealt to `lanes`
    CONTIGUOUS blocks whose sketches advance in lock-step inside the same launches.  A block is preceded by ONE halo window
    it does not own (MAIN(t) continues AUX(t - 1), AUX starts empty: the sequential sketch is reproduced exactly); the block
    that starts at the beginning of the stream gets a window of empty rows instead.  R (main.py:61) is fixed by stream window
    0.  Raw k-means labels are collected per window and the Hungarian chain (main.py:105-119) is replayed in stream order.

        lanes = SwfdmcLanes(W, l, k, seed, n_lanes, R)      # R = max out-degree of window 0's fused adjacency
        out = lanes.run(windows, labels)                     # windows[t] = list of modality tensors of stream window t
    """

    def __init__(self, W, ell, k, seed, lanes, R, modality_types=None, stream=None, assume_finite=False, modality_weights=None,
                 fusion_threshold=None, modality_ks=None):
        from .swfd import SeqBasedSWFD

        # `fusion_threshold`: the sketch ingests the bit rows of the thresholded mask (weights then only weight the vote);
        # `modality_ks`: one k per modality -- both as for StreamPipeline, which fuses for the lanes
        if modality_weights is not None and fusion_threshold is None:
            raise ValueError("modality_weights: the SWFD sketch ingests the bit rows of the OR-fused adjacency")

        self.W, self.ell, self.k, self.seed, self.lanes = int(W), int(ell), int(k), int(seed), int(lanes)
        self.types = list(modality_types) if modality_types else None
        self.pipe = StreamPipeline(W, ell, k, seed, "sSVDMC", modality_types=self.types, async_labels=True, stream=stream,
                                   assume_finite=assume_finite, modality_weights=modality_weights,
                                   fusion_threshold=fusion_threshold, modality_ks=modality_ks)
        self.sk = SeqBasedSWFD(N=self.W, R=float(R), d=self.W, sketch_dim=self.ell, lanes=self.lanes)
        self.words = (self.W + 63) // 64
        self._masks = torch.zeros((self.lanes, self.W, self.words), dtype=torch.int64, device="cuda")

    @staticmethod
    def r_of_first_window(mods, W, k, modality_types=None, seed=0, modality_weights=None, fusion_threshold=None,
                          modality_ks=None):
        """main.py:61 on the fused adjacency of stream window 0 (fused as the lanes will fuse it: give the same
        `fusion_threshold`, vote weights and `modality_ks`)."""
        if modality_weights is not None and fusion_threshold is None:
            raise ValueError("modality_weights: the SWFD sketch ingests the bit rows of the OR-fused adjacency")
        with StreamPipeline(W, 2, k, seed, "sSVDMC", modality_types=modality_types, async_labels=False,
                            modality_weights=modality_weights, fusion_threshold=fusion_threshold, modality_ks=modality_ks) as p:
            types, ks = p.types or [""] * len(mods), p._ks(len(mods))
            adjs = [p._adjacency(_to_dev(m), t, k=ks[i]) for i, (m, t) in enumerate(zip(mods, types))]
            return p.eng.max_row_sq_norm(p._fuse_binary(adjs))

    def step(self, mods_per_lane, labels_per_lane, triggers, want):
        """One lock-step: lane p appends the fused adjacency of mods_per_lane[p] (None: a window of empty rows); lanes with
        want[p] get their window's sketch, k-means and a trace entry under triggers[p]."""
        eng, types = self.pipe.eng, None
        for p, mods in enumerate(mods_per_lane):
            if mods is None:
                self._masks[p].zero_()
                continue
            types = self.types or [""] * len(mods)
            eng.begin_window(False)
            ks = self.pipe._ks(len(mods))
            adjs = [self.pipe._adjacency(_to_dev(m), t, k=ks[i]) for i, (m, t) in enumerate(zip(mods, types))]
            self._masks[p].copy_(self.pipe._fuse_binary(adjs, eng).mask)
        self.sk.fit_adjacency_lanes(self._masks)
        if not any(want):
            return
        B, sigma, _ = self.sk.get_device()                     # (lanes, l, W)
        for p in range(self.lanes):
            if want[p]:
                reduced = B[p].t().contiguous()                # main.py:73-76: (W, l)
                self.pipe.process_reduced(reduced, sigma[p], labels_per_lane[p], trigger=triggers[p])

    def run(self, windows, labels):
        """windows: list over stream windows of lists of modality arrays / tensors (W rows each); labels: true labels per
        window.  Returns all_clusters in stream order (the concatenated matched labels)."""
        from . import distributed as mdist

        K = len(windows)
        if K < self.lanes:
            raise ValueError(f"{self.lanes} lanes need at least as many windows (got {K})")
        for row in mdist.lane_schedule(K, self.lanes):
            mods = [windows[i] if i >= 0 else None for i, _ in row]
            labs = [labels[i] if i >= 0 else None for i, _ in row]
            self.step(mods, labs, [i for i, _ in row], [own for _, own in row])
        self.pipe.flush()
        self.sk.check()
        raw = {tr["trigger"]: tr["raw"] for tr in self.pipe.trace}
        self.sigma = {tr["trigger"]: tr["sigma"] for tr in self.pipe.trace}
        raw = np.array([raw[t] for t in range(K)], dtype=np.int64)
        if self.pipe._match_device:   # the whole chain in one launch (csrc/match_hung.hip); MUSED_MATCH=host: SciPy per window
            return mo.match_chain_on_device(raw, method="hungarian", wide=True)
        return mdist.replay_label_chain(raw, mo.match_clusters)

    def close(self):
        self.pipe.close()
        self.sk.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _to_dev(m):
    return m if isinstance(m, torch.Tensor) or not isinstance(m, np.ndarray) or m.dtype.kind not in "fiu" else torch.from_numpy(m).cuda()
