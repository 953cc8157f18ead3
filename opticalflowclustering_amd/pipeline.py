"""Device-resident clip pipeline (BASELINE.json configs[2]/[3]): a clip's frames sit in HBM, dense
Farneback flow is computed for every consecutive pair in batches, and Lloyd's k-means runs over the
per-pixel (u,v) vectors of the whole clip without the flow ever leaving the device.  With a
communicator (dist.py) each rank owns a contiguous range of pairs (plus the one-frame halo) and the
Lloyd partial sums are all-reduced over RCCL once per iteration."""
import ctypes as C

import numpy as np

from . import _lib, stages
from ._lib import DeviceBuffer, FbParams, check, load
from .cluster import kmeans_fit_dev, kmeans_plusplus_dev
from .flow import FlowEngine


def shard_pairs(n_pairs, world, rank):
    """contiguous ranges of pair indices, sizes differing by at most one"""
    base, rem = divmod(n_pairs, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def batch_schedule(n_pairs, batch_pairs):
    """sizes of the flow launch sequences a clip of n_pairs is cut into.  batch_pairs: pairs per batch, or an explicit schedule.
    The short batch goes FIRST: at the end of a step both engines then finish on full batches instead of one of them running
    a half-empty launch sequence alone (36.7 against 37.0 ms per 299-pair step)"""
    if isinstance(batch_pairs, (list, tuple)):
        schedule = [int(b) for b in batch_pairs]
        if sum(schedule) != n_pairs or min(schedule) < 1:
            raise ValueError(f"batch schedule {schedule} does not cover {n_pairs} pairs")
        return schedule
    b = max(1, min(int(batch_pairs), n_pairs))
    return ([n_pairs % b] if n_pairs % b else []) + [b] * (n_pairs // b)


class ClipPipeline:
    def __init__(self, W, H, n_frames_local, batch_pairs=16, params=None, device=0, n_engines=2):
        self.W, self.H, self.device = W, H, device
        self.n_frames = int(n_frames_local)
        self.n_pairs = self.n_frames - 1
        self.schedule = batch_schedule(self.n_pairs, batch_pairs)
        self.batch = max(self.schedule)
        # two engines = two HIP streams: consecutive batches are independent, so their kernels overlap and fill
        # each other's tails / latency-bound phases
        self.engines = [FlowEngine(W, H, params or FbParams(), max_batch=self.batch, device=device)
                        for _ in range(max(1, min(n_engines, len(self.schedule))))]
        self.engine = self.engines[0]
        P = W * H
        self.frames = DeviceBuffer(self.n_frames * P, device)
        self.flows = DeviceBuffer(self.n_pairs * P * 8, device)
        self.labels = DeviceBuffer(self.n_pairs * P, device)
        # sum(u), sum(v) per batch, written by the flow engine with the field (epilogue of the last level-0 iteration):
        # run_kmeans adds them up in batch order instead of sweeping the 5 GB of vectors once more for the column means
        self.n_batches = len(self.schedule)
        self.uv_sums = DeviceBuffer(self.n_batches * 16, device)
        self._sums_valid = False
        self.weights = None                 # N f32 sample weights for run_kmeans, allocated on first use
        self._label_k = None                # the k the resident labels were written with (run_kmeans / assign), or None
        self.moves = None                   # capture_moves(): the move words of the field as it was then, n_pairs * P int32
        self._compensated = False           # compensate_camera() has run since the last run_flow()
        self.frames_rev = None              # run_backward_flow(): the resident frames in reverse order, n_frames * P u8
        self.flows_bwd = None               # ... and the field of that clip: pair t's backward field at n_pairs-1-t
        self.bwd_reversed = True            # False after run_flow_bidirectional(): pair t's backward field at t
        self.state = None                   # consistency() / photometric(): the state map of the check that ran last, n_pairs * P u8
        self.filled = None                  # repair(): the round every pixel was filled in, n_pairs * P u8

    def synth(self, t0=0, seed=0):
        """fill the resident clip with synthetic frames t0 .. t0+n_frames-1"""
        check(load().ofc_synth_frames_dev(self.device, C.c_void_p(self.frames.ptr), self.W, self.H,
                                          self.n_frames, t0, seed))

    def upload_frames(self, frames):
        frames = np.ascontiguousarray(frames, np.uint8)
        assert frames.shape == (self.n_frames, self.H, self.W)
        self.frames.upload(frames)

    def run_flow(self, sync=True, stats=True):
        P = self.W * self.H
        p0 = 0
        for i, n in enumerate(self.schedule):
            self.engines[i % len(self.engines)].calc_frames_dev(self.frames.ptr + p0 * P, n + 1,
                                                                self.flows.ptr + p0 * P * 8, sync=False,
                                                                uv_sum_ptr=self.uv_sums.ptr + 16 * i if stats else None)
            p0 += n
        self._sums_valid = stats
        self._label_k = None                # the labels belong to the field that was just overwritten
        self._compensated = False
        if self.moves is not None:          # ... and so do the captured moves
            self.moves.free()
            self.moves = None
        self._drop_backward()               # ... and the backward field and the state map checked against it
        if sync:
            self.sync()

    def _drop_backward(self):
        for name in ("frames_rev", "flows_bwd", "state", "filled"):
            b = getattr(self, name)
            if b is not None:
                b.free()
                setattr(self, name, None)

    def run_backward_flow(self, sync=True):
        """the backward field of every resident pair, for consistency(): the resident frames are copied in reverse order into
        a buffer of the pipeline's own (consistency.frames_reverse_dev) and the flow runs over that clip with run_flow()'s
        schedule on the same engines, into flows_bwd.  Pair t of that field is frame n-1-t -> n-2-t, so the backward field
        of forward pair t sits at n_pairs-1-t (the library's bwd_reversed = 1).  Costs what run_flow() costs, and as much
        memory again for the field.  run_flow() discards it."""
        from . import consistency as cons
        P = self.W * self.H
        self.sync()
        self._drop_backward()
        self.frames_rev = DeviceBuffer(self.n_frames * P, self.device)
        self.flows_bwd = DeviceBuffer(self.n_pairs * P * 8, self.device)
        self.bwd_reversed = True
        cons.frames_reverse_dev(self.frames.ptr, self.W, self.H, self.n_frames, self.frames_rev.ptr, self.device)
        p0 = 0
        for i, n in enumerate(self.schedule):
            self.engines[i % len(self.engines)].calc_frames_dev(self.frames_rev.ptr + p0 * P, n + 1,
                                                                self.flows_bwd.ptr + p0 * P * 8, sync=False)
            p0 += n
        if sync:
            self.sync()

    def run_flow_bidirectional(self, sync=True):
        """run_flow() and the backward field of every pair from ONE front end (FlowEngine.calc_frames_dev_bidir): the same
        batch schedule on the same engines, forward fields into the resident field as run_flow() leaves them, backward fields
        into flows_bwd in the clip's own order (pair t's at t: the library's bwd_reversed = 0, which consistency() then
        passes).  The column sums for run_kmeans come from a sweep over each batch's finished forward field.  As much memory
        again for the field; the next run_flow() discards it."""
        P = self.W * self.H
        self.sync()
        self._drop_backward()
        self.flows_bwd = DeviceBuffer(self.n_pairs * P * 8, self.device)
        p0 = 0
        for i, n in enumerate(self.schedule):
            self.engines[i % len(self.engines)].calc_frames_dev_bidir(self.frames.ptr + p0 * P, n + 1, self.flows.ptr + p0 * P * 8,
                                                                      self.flows_bwd.ptr + p0 * P * 8, sync=False,
                                                                      uv_sum_ptr=self.uv_sums.ptr + 16 * i)
            p0 += n
        self.bwd_reversed = False
        self._sums_valid = True
        self._label_k = None                # as run_flow(): labels, camera and moves belonged to the overwritten field
        self._compensated = False
        if self.moves is not None:
            self.moves.free()
            self.moves = None
        if sync:
            self.sync()

    def flows_bwd_host(self):
        """host copy of the backward field in the order it has on the device: the reversed clip's after run_backward_flow()
        (pair t's at n_pairs-1-t), the clip's own after run_flow_bidirectional() (pair t's at t); bwd_reversed says which"""
        if self.flows_bwd is None:
            raise ValueError("no backward field: call run_backward_flow() first (run_flow() discards it)")
        self.sync()
        return self.flows_bwd.download((self.n_pairs, self.H, self.W, 2), np.float32)

    def consistency(self, alpha=0.01, beta=0.5, residual=False):
        """the forward-backward check of the resident field against the backward field of run_backward_flow() or
        run_flow_bidirectional(), in whichever order that left it (consistency.py; ofc_consist_dev)
        -> consistency.Consistency.  The state map also stays on the device, for blobs(consistent=True) and
        run_kmeans / seed_kmeans(consistent=True), until the next run_flow().  alpha, beta: consistency.check's, a
        convention of the literature and not tuned here.  ValueError without a backward field, and after
        compensate_camera(): a residual does not say where a pixel lands (the rule blobs(links=) has), so check before the
        camera is removed.  Rank-local: a pair depends on itself alone."""
        from . import consistency as cons
        alpha_q, beta_q = cons.quantise(alpha, beta)
        if self.flows_bwd is None:
            raise ValueError("consistency() needs the backward field: call run_backward_flow() first (run_flow() discards it)")
        if self._compensated:
            raise ValueError("consistency() after compensate_camera() would follow the residual, which does not say where a "
                             "pixel lands: call it before compensate_camera()")
        self.sync()
        n, W, H = self.n_pairs, self.W, self.H
        if self.state is None:
            self.state = DeviceBuffer(n * W * H, self.device)
        try:
            counts, resid = cons.check_dev(self.flows.ptr, self.flows_bwd.ptr, W, H, n, self.state.ptr, alpha_q, beta_q,
                                           bwd_reversed=self.bwd_reversed, residual=residual, device=self.device)
        except Exception:
            self.state.free()
            self.state = None
            raise
        return cons.Consistency(self.state.download((n, H, W), np.uint8), counts, resid, alpha_q, beta_q)

    def photometric(self, tau=8.0, kappa=0.5, warped=False):
        """the photometric check of the resident field against the resident frames (photometric.py; ofc_photo_dev), in
        chunks of at most 65535 pairs -> photometric.Photometric.  It needs no backward field.  The state map also stays on
        the device, where consistency() leaves its own: whichever of the two ran last owns it, and blobs(consistent=True)
        and run_kmeans / seed_kmeans(consistent=True) take it unchanged, until the next run_flow().  tau, kappa:
        photometric.check's, a convention that is not tuned on anything here.  ValueError after compensate_camera(): a
        residual does not say where a pixel lands (the rule consistency() has), so check before the camera is removed.
        Rank-local: a pair depends on itself and its two frames alone."""
        from . import photometric as photo
        tau_q, kappa_q = photo.quantise(tau, kappa)
        if self._compensated:
            raise ValueError("photometric() after compensate_camera() would follow the residual, which does not say where a "
                             "pixel lands: call it before compensate_camera()")
        self.sync()
        n, W, H = self.n_pairs, self.W, self.H
        P = W * H
        photo.check_args(W, H, min(n, 65535), tau_q, kappa_q)
        if self.state is None:
            self.state = DeviceBuffer(n * P, self.device)
        stats, out = [], []
        try:
            for t0 in range(0, n, 65535):
                m = min(65535, n - t0)
                st, wd = photo.check_dev(self.frames.ptr + t0 * P, self.flows.ptr + t0 * P * 8, W, H, m, self.state.ptr + t0 * P,
                                         tau_q, kappa_q, warped=warped, device=self.device)
                stats.append(st)
                out.append(wd)
        except Exception:
            self.state.free()
            self.state = None
            raise
        return photo.Photometric(self.state.download((n, H, W), np.uint8), np.concatenate(stats),
                                 np.concatenate(out) if warped else None, tau_q, kappa_q)

    def repair(self, radius=1, rounds=8, min_count=1, smooth=False, keep=(0,), need_state=True):
        """the masked median fill of the resident field, in place (repair.py; ofc_repair_dev), in chunks of at most 65535
        pairs -> (n,3) int64, every pair's sources, filled and unfilled pixels.  The sources are the pixels whose state in
        the map that consistency() or photometric() left is in `keep` (consistency.keep_mask); ValueError when there is no
        such map (need_state=False: then only the vectors that are not usable numbers are filled).  Every other pixel is replaced by the median of the sources around it, round after round; smooth adds a
        median pass over the whole field.  The state map is updated: a filled pixel becomes CONSISTENT, so
        blobs(consistent=True) and run_kmeans / seed_kmeans(consistent=True) take it back in.  The round every pixel was
        filled in stays on the device: filled_host().  rounds and min_count default to 8 and 1, a convention, not tuned
        on anything here.  ValueError after compensate_camera(): a repaired vector says where a pixel lands, so
        repair before the camera is removed.  The batch sums of the flow no longer describe the field afterwards, so
        run_kmeans sweeps it for its column means.  Rank-local: a pair depends on itself alone."""
        from . import repair as rep
        kp = rep.keep_mask(keep)
        if self.state is None and need_state:
            raise ValueError("repair() needs the state map of a check: call photometric(), or run_backward_flow() and "
                             "consistency(), first (run_flow() discards them)")
        if self._compensated:
            raise ValueError("repair() after compensate_camera() would fill the residual, which does not say where a pixel "
                             "lands: call it before compensate_camera()")
        self.sync()
        n, W, H = self.n_pairs, self.W, self.H
        P = W * H
        rep.check_args(W, H, min(n, 65535), kp, radius, rounds, min_count, smooth)
        if self.filled is None:
            self.filled = DeviceBuffer(n * P, self.device)
        counts = []
        for t0 in range(0, n, 65535):
            m = min(65535, n - t0)
            st = self.state.ptr + t0 * P if self.state is not None else None
            counts.append(rep.fill_dev(self.flows.ptr + t0 * P * 8, st, W, H, m, None, self.filled.ptr + t0 * P, st, kp, radius,
                                       rounds, min_count, smooth, self.device))
        self._sums_valid = False
        self._label_k = None                # the labels belong to the field as it was
        return np.concatenate(counts)

    def trajectories(self, seeds=None, step=8, start=0, length=None, consistent=False, keep=(0,), pairs_per_launch=0):
        """follow points through the resident field (trajectories.py; ofc_traj_dev) -> trajectories.Trajectories.  seeds:
        int32 (P,2) in 1/65536 px, None for trajectories.grid_seeds(W, H, step); the points are placed at pair `start` and
        followed through `length` pairs (None: to the end of the clip): a sub-range is a pointer offset into the field.
        consistent=True: a point ends where the state map that consistency() or photometric() left (and repair() updated)
        is not in `keep`; ValueError without one.  ValueError after compensate_camera(): a residual does not say where a
        pixel lands (the rule consistency() has), so follow before the camera is removed.  Rank-local: this rank's pairs."""
        from . import trajectories as tr
        if self._compensated:
            raise ValueError("trajectories() after compensate_camera() would follow the residual, which does not say where a "
                             "pixel lands: call it before compensate_camera()")
        start = int(start)
        n = self.n_pairs - start if length is None else int(length)
        if not (0 <= start < self.n_pairs and 1 <= n <= self.n_pairs - start):
            raise ValueError(f"start = {start}, length = {length!r}: a range of the clip's {self.n_pairs} pairs")
        state_ptr = self._state_ptr("trajectories(consistent=True)") if consistent else None
        self.sync()
        P = self.W * self.H
        return tr.follow_dev(self.flows.ptr + start * P * 8, self.W, self.H, n, tr._seeds(seeds, self.W, self.H, step),
                             state_ptr=state_ptr + start * P if consistent else None, keep=keep, pairs_per_launch=pairs_per_launch,
                             device=self.device)

    def tracklets(self, cell=8, length=15, max_tracks=None, start=0, pairs=None, consistent=False, keep=(0,)):
        """dense trajectories with reseeding on the resident field (trajectories.follow_dense; ofc_tracklets_dev) ->
        trajectories.Tracklets: every frame each cell x cell grid cell without a live track gets a new one, and a track is
        cut after `length` steps.  The clip starts at pair `start` and has `pairs` pairs (None: to the end): a sub-range is
        a pointer offset into the field.  max_tracks None: trajectories.default_max_tracks for the range.  consistent=True
        and the refusals as trajectories().  Rank-local: this rank's pairs."""
        from . import trajectories as tr
        if self._compensated:
            raise ValueError("tracklets() after compensate_camera() would follow the residual, which does not say where a "
                             "pixel lands: call it before compensate_camera()")
        start = int(start)
        n = self.n_pairs - start if pairs is None else int(pairs)
        if not (0 <= start < self.n_pairs and 1 <= n <= self.n_pairs - start):
            raise ValueError(f"start = {start}, pairs = {pairs!r}: a range of the clip's {self.n_pairs} pairs")
        state_ptr = self._state_ptr("tracklets(consistent=True)") if consistent else None
        self.sync()
        P = self.W * self.H
        return tr.follow_dense_dev(self.flows.ptr + start * P * 8, self.W, self.H, n, cell=cell, length=length, max_tracks=max_tracks,
                                   state_ptr=state_ptr + start * P if consistent else None, keep=keep, device=self.device)

    def filled_host(self):
        """host copy of repair()'s map: (n,H,W) u8, 0 for a source, g for a pixel filled in round g, 255 for one never filled"""
        if self.filled is None:
            raise ValueError("no filled map: call repair() first (run_flow() discards it)")
        return self.filled.download((self.n_pairs, self.H, self.W), np.uint8)

    def _state_ptr(self, what):
        if self.state is None:
            raise ValueError(f"{what} needs the state map of the forward-backward check: call run_backward_flow() and "
                             "consistency() first (run_flow() discards them)")
        return self.state.ptr

    def sync(self):
        for e in self.engines:
            e.sync()

    def _weights_ptr(self, sample_weight, N, consistent=False):
        if consistent:
            state_ptr = self._state_ptr("consistent=True")
            if sample_weight is None:
                sample_weight = ("moving", 0.0)
        if sample_weight is None:
            return None
        if self.weights is None:
            self.weights = DeviceBuffer(N * 4, self.device)
        if isinstance(sample_weight, str) or isinstance(sample_weight, tuple):
            kind, thr = (sample_weight, 0.0) if isinstance(sample_weight, str) else sample_weight
            if kind not in ("magnitude", "moving") or (kind == "moving") != isinstance(sample_weight, tuple):
                raise ValueError("sample_weight should be None, 'magnitude', ('moving', thr) or an array, "
                                 f"got {sample_weight!r}")
            stages.flow_weights_dev(self.flows.ptr, N, kind, thr, self.weights.ptr, self.device)
        else:
            w = np.ascontiguousarray(sample_weight, np.float32).ravel()
            if w.shape != (N,):
                raise ValueError(f"sample_weight has {w.size} entries, expected {N}")
            if not np.isfinite(w).all() or (w < 0).any():
                raise ValueError("sample_weight must be finite and >= 0")
            self.weights.upload(w)
        if consistent:                      # a pixel that failed the check counts for nothing
            from . import consistency as cons
            cons.mask_dev(state_ptr, N, w_ptr=self.weights.ptr, device=self.device)
        return self.weights.ptr

    def _colsum(self):
        if not self._sums_valid:
            return None
        per_batch = self.uv_sums.download((self.n_batches, 2), np.float64)
        colsum = np.zeros(2)
        for b in range(self.n_batches):                 # fixed order
            colsum += per_batch[b]
        return colsum

    def seed_kmeans(self, k, random_state=None, n_global=None, sample_weight=None, consistent=False):
        """sklearn's k-means++ seeding on the resident (u,v) vectors (cluster.kmeans_plusplus_dev), with sample_weight as
        in run_kmeans: the weights then decide the first centre, every later draw and every candidate's potential, as in
        sklearn's fit(X, sample_weight=).  run_kmeans(C0, sample_weight=...) from the returned centres completes that fit.
        None gives the seeds run_kmeans('k-means++', k=k) starts from.  consistent as in run_kmeans.
        -> (centers (k,2), GLOBAL indices)"""
        self.sync()
        N = self.n_pairs * self.W * self.H
        wptr = self._weights_ptr(sample_weight, N, consistent)
        return kmeans_plusplus_dev(self.flows.ptr, _lib.F32, N, 2, int(k), random_state, device=self.device,
                                   colsum=self._colsum(), n_global=n_global, weights_ptr=wptr, weight_dtype=_lib.F32)

    def run_kmeans(self, init, max_iter=300, tol=1e-4, k=None, random_state=None, n_global=None, sample_weight=None,
                   consistent=False):
        """Lloyd over all local (u,v) vectors (global when a communicator is active).
        init: (k,2) array, or 'k-means++' with k= and random_state=: sklearn's seeding on the resident vectors
        (cluster.kmeans_plusplus_dev).  Under a communicator every rank passes the same random_state, and n_global = the
        number of (u,v) vectors over all ranks.
        sample_weight: None, 'magnitude' (a vector counts by its length), ('moving', thr) (1 where the length reaches thr,
        else 0), or one value per local vector (kept as f32).  The weights live in a device buffer allocated on first use;
        not available together with init='k-means++' in one call (seed_kmeans(k, sample_weight=...) first, then pass its
        centres as init).
        consistent=True: the weight of every pixel whose state in consistency()'s map is not CONSISTENT becomes 0
        (ofc_consist_mask_dev on the weight buffer); with sample_weight=None the weights start from ('moving', 0.0).  It
        makes the fit a weighted one, so the rule about init='k-means++' applies.  -> centers (k,2), inertia, n_iter"""
        self.sync()
        N = self.n_pairs * self.W * self.H
        if (sample_weight is not None or consistent) and isinstance(init, str):
            raise ValueError("sample_weight or consistent=True together with init='k-means++' is not supported in one call: seed "
                             "first, C0, _ = seed_kmeans(k, random_state, sample_weight=...), then run_kmeans(C0, sample_weight=...)")
        wptr = self._weights_ptr(sample_weight, N, consistent)
        colsum = self._colsum()
        if isinstance(init, str):
            if init != "k-means++" or k is None:
                raise ValueError(f"init should be a (k,2) array or 'k-means++' together with k=, got {init!r}, k={k!r}")
            init, _ = kmeans_plusplus_dev(self.flows.ptr, _lib.F32, N, 2, int(k), random_state, device=self.device,
                                          colsum=colsum, n_global=n_global)
        self._label_k = None
        fit = kmeans_fit_dev(self.flows.ptr, _lib.F32, N, 2, init, max_iter, tol, self.labels.ptr, self.device, colsum=colsum,
                             weights_ptr=wptr, weight_dtype=_lib.F32, field=(self.W, self.H))
        self._label_k = len(fit[0])
        return fit

    def _centred_model(self, centers):
        """-> (k, the resident field's column mean (2,), centres minus that mean (k,2)): what assign labels against"""
        self.sync()
        cen = np.ascontiguousarray(centers, np.float64)
        if cen.ndim != 2 or cen.shape[1] != 2 or len(cen) < 1:
            raise ValueError(f"centers should be a (k,2) array, got shape {cen.shape}")
        N = self.n_pairs * self.W * self.H
        colsum = self._colsum()
        if colsum is None:
            colsum = np.empty(2, np.float64)
            check(load().ofc_lloyd_colstats_dev(self.device, C.c_void_p(self.flows.ptr), _lib.F32, N, 2, None, 0,
                                                _lib.ptr(colsum)))
        mean = np.ascontiguousarray(colsum / N)
        return len(cen), mean, np.ascontiguousarray(cen - mean)

    def assign(self, centers):
        """label the resident (u,v) vectors against the given (k,2) centres without fitting (a model fitted on another
        clip, say): one E-step (ofc_lloyd_step_dev, nothing accumulated), centred by this field's own column mean as the
        fit's final E-step is.  The labels replace the resident ones; cell_clusters() summarises them.  Under a
        communicator this is rank-local: this rank's pairs, this rank's mean, no collective."""
        k, mean, cen_c = self._centred_model(centers)
        N = self.n_pairs * self.W * self.H
        self._label_k = None
        check(load().ofc_lloyd_step_dev(self.device, C.c_void_p(self.flows.ptr), _lib.F32, N, 2, k, _lib.ptr(mean),
                                        _lib.ptr(cen_c), C.c_void_p(self.labels.ptr), 0, None))
        self._label_k = k

    def cell_clusters(self, rows=14, cols=25, sums=False, centers=None):
        """what the resident labels say per grid cell (ofc_grid_label_counts_dev, the grid of KmeanGrids.py:56-59):
        counts (n_pairs, rows*cols, k) int32 = pixels of the cell in each cluster, and with sums=True also
        (n_pairs, rows*cols, k, 2) f64 = the sums of their (u, v); only these few numbers leave the device.
        Needs labels: after run_kmeans() or assign(), not after a run_flow() that replaced the field.
        With centers= ((k,2), a model fitted elsewhere) the result is that of assign(centers) followed by
        cell_clusters(rows, cols, sums), from one sweep of the field (ofc_grid_assign_counts_dev): every vector is
        labelled as assign labels it, centred by this field's own mean, and counted at once.  The resident labels are
        neither needed nor touched, and stay those of the last run_kmeans() / assign().
        Under a communicator the result covers this rank's pairs; the ranks' rows concatenated in rank order are the
        single-rank result (a pair's rows depend on that pair alone), so no collective is involved."""
        if centers is not None:
            k, mean, cen_c = self._centred_model(centers)
        elif self._label_k is None:
            raise ValueError("cell_clusters needs labels for the resident field: call run_kmeans() or assign() first "
                             "(run_flow() discards them)")
        else:
            k = self._label_k
        n = self.n_pairs
        nout = max(n * int(rows) * int(cols) * k, 1)      # the library refuses a grid that does not fit
        cnt = DeviceBuffer(nout * 4, self.device)
        sm = DeviceBuffer(nout * 16, self.device) if sums else None
        try:
            if centers is not None:
                check(load().ofc_grid_assign_counts_dev(self.device, C.c_void_p(self.flows.ptr), self.W, self.H, n, rows,
                                                        cols, k, _lib.ptr(mean), _lib.ptr(cen_c), C.c_void_p(cnt.ptr),
                                                        C.c_void_p(sm.ptr) if sums else None))
            else:
                check(load().ofc_grid_label_counts_dev(self.device, C.c_void_p(self.labels.ptr),
                                                       C.c_void_p(self.flows.ptr) if sums else None, self.W, self.H, n, rows,
                                                       cols, k, C.c_void_p(cnt.ptr), C.c_void_p(sm.ptr) if sums else None))
            counts = cnt.download((n, rows * cols, k), np.int32)
            return (counts, sm.download((n, rows * cols, k, 2), np.float64)) if sums else counts
        finally:
            cnt.free()
            if sm is not None:
                sm.free()

    def uv_histogram(self, bins=1024, range=32.0):
        """the (u,v) histogram of the resident field (ofc_uv_hist_accum_dev: one read of the field where the flow left it;
        only the table leaves the device) -> uvhist.UVHistogram, whose fit() stands in for run_kmeans on this field and
        takes n_init restarts.  Rank-local: this rank's pairs, no collective; the ranks' tables merge by addition."""
        from .uvhist import UVHistogram, check_params, table_len
        bins, range = check_params(bins, range)
        self.sync()
        tab = DeviceBuffer(table_len(bins) * 8, self.device)
        try:
            tab.zero()
            check(load().ofc_uv_hist_accum_dev(self.device, C.c_void_p(self.flows.ptr), self.n_pairs * self.W * self.H, bins,
                                               range, C.c_void_p(tab.ptr)))
            return UVHistogram(bins, range, tab.download((table_len(bins),), np.int64))
        finally:
            tab.free()

    def compensate_camera(self, model="affine", thresholds=(4.0, 2.0, 1.0)):
        """fit every pair's camera motion on the resident field and subtract it there (camera.py: ofc_motion_fit_dev, then
        ofc_motion_subtract_dev in place) -> camera.CameraMotion.  What follows -- run_kmeans and its weights, uv_histogram,
        assign, cell_clusters(centers=) -- then sees the motion against the background.  The flow engine's column sums
        and the resident labels belong to the field as it was: the next fit sweeps for its own column sums, and
        cell_clusters() without centers= is refused until run_kmeans() or assign() has labelled the residual.
        The default thresholds are a guess, not tuned on any footage.  Rank-local under a communicator: a pair depends on
        itself alone, no collective."""
        from . import camera as cam
        kind, thr, T = cam.camera_args(model, thresholds)
        self.sync()
        n = self.n_pairs
        params, status = np.zeros((n, 6)), np.zeros(n, np.int32)
        moments = np.zeros((T + 1, n, cam.NMOM), np.int64)
        fp = C.c_void_p(self.flows.ptr)
        check(load().ofc_motion_fit_dev(self.device, fp, self.W, self.H, n, kind, _lib.ptr(thr), T, _lib.ptr(params),
                                        _lib.ptr(status), None, _lib.ptr(moments)))
        self._sums_valid = False
        self._label_k = None
        self._compensated = True
        check(load().ofc_motion_subtract_dev(self.device, fp, self.W, self.H, n, _lib.ptr(params), fp))
        return cam.motion_from_history(params, status, moments, model)

    def capture_moves(self):
        """store where the resident field says every pixel goes (blobs.moves_dev: its vectors rounded to whole pixels, one
        int32 each, on the device) for blobs(links=).  Call it before compensate_camera(): the residual does not say where
        a pixel lands.  run_flow() discards what was captured."""
        from . import blobs as bl
        self.sync()
        if self.moves is None:
            self.moves = DeviceBuffer(self.n_pairs * self.W * self.H * 4, self.device)
        bl.moves_dev(self.flows.ptr, self.W, self.H, self.n_pairs, self.moves.ptr, self.device)

    def blobs(self, by="moving", thr=0.5, select=None, merge=False, connectivity=8, min_area=1, max_blobs=4096, labels=True,
              mean="field", links=None, consistent=False):
        """the moving objects of every resident pair (blobs.py: connected components of a key map, one record each) ->
        blobs.Blobs.  by='moving': the pixels whose vector's length reaches thr, all with key 0 (on hand-held footage call
        compensate_camera first).  by='labels': the label buffer of the last run_kmeans() / assign() is the key map as it
        stands; thr, select and merge do not apply.  by=centers ((k,2), a model fitted elsewhere): every vector is keyed by
        the label assign(centers) would give it, centred by this field's own mean (mean='field'; mean=None labels un-centred,
        as a FlowStream's model does, or pass the two values); select (labels to keep, None = all),
        merge (join neighbouring regions of different labels) and thr (None: no motion test) as blobs.cluster_blobs.
        The records' mean flow comes from the resident field.  Rank-local: a pair depends on itself alone.
        links = a max_links: the blobs of consecutive pairs are linked as well (Blobs.links, Blobs.nlinks; blobs.tracks turns
        them into track ids), by the moves capture_moves() stored, or, where none were captured, by moves taken from the
        resident field as it stands; ValueError if compensate_camera() has run since the last run_flow() and no moves were
        captured, because the residual does not say where a pixel goes.  Links are rank-local too: a transition whose two
        pairs live on different ranks is not linked.
        consistent=True: the key map is masked to the pixels that consistency() found CONSISTENT before the components are
        found (ofc_consist_mask_dev: every other pixel becomes background).  ValueError with by='labels', whose key map is
        the label buffer itself, and without a state map."""
        from . import blobs as bl
        self.sync()
        n, W, H = self.n_pairs, self.W, self.H
        if consistent:
            if isinstance(by, str) and by == "labels":
                raise ValueError("blobs(by='labels', consistent=True): that key map is the label buffer itself and is not "
                                 "masked; key by 'moving' or by centres")
            state_ptr = self._state_ptr("blobs(consistent=True)")
        link = {}
        if links is not None:
            if self.moves is None and self._compensated:
                raise ValueError("blobs(links=) after compensate_camera() needs the moves of the whole flow: call "
                                 "capture_moves() before compensate_camera()")
            link = dict(links=int(links), moves_ptr=self.moves.ptr if self.moves is not None else None)
        if isinstance(by, str) and by == "labels":
            if self._label_k is None:
                raise ValueError("blobs(by='labels') needs labels for the resident field: call run_kmeans() or assign() first "
                                 "(run_flow() discards them)")
            return bl.components_dev(self.labels.ptr, self.flows.ptr, W, H, n, connectivity, min_area, max_blobs, labels, self.device,
                                     **link)
        bl.check_args(W, H, n, connectivity, min_area, max_blobs)
        keys = DeviceBuffer(n * W * H, self.device)
        try:
            if isinstance(by, str):
                if by != "moving":
                    raise ValueError(f"by should be 'moving', 'labels' or a (k,2) array of centres, got {by!r}")
                bl.keys_dev(self.flows.ptr, W, H, n, keys.ptr, thr=thr, device=self.device)
            else:
                if isinstance(mean, str):
                    _, mean, _ = self._centred_model(by)
                bl.keys_dev(self.flows.ptr, W, H, n, keys.ptr, thr=thr, centers=by, mean=mean, select=select, merge=merge,
                            device=self.device)
            if consistent:
                from . import consistency as cons
                cons.mask_dev(state_ptr, n * W * H, keys_ptr=keys.ptr, device=self.device)
            out = bl.components_dev(keys.ptr, self.flows.ptr, W, H, n, connectivity, min_area, max_blobs, labels, self.device,
                                    **link)
            out.keys = keys.download((n, H, W), np.uint8)
            return out
        finally:
            keys.free()

    def sample_uv(self, idx):
        """host copy of a few (u,v) rows (for choosing the initial centres)"""
        out = np.empty((len(idx), 2), np.float32)
        for i, j in enumerate(idx):
            out[i] = self.flows.download((2,), np.float32, offset=int(j) * 8)
        return out

    def flows_host(self):
        return self.flows.download((self.n_pairs, self.H, self.W, 2), np.float32)

    def labels_host(self):
        return self.labels.download((self.n_pairs, self.H, self.W), np.uint8)

    def close(self):
        for e in self.engines:
            e.close()
        self._drop_backward()
        for b in (self.frames, self.flows, self.labels, self.uv_sums, self.weights, self.moves):
            if b is not None:
                b.free()
