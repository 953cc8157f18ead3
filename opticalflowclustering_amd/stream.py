"""Streaming ingest (BASELINE.json configs[4] shape): frames are pushed one at a time (as a decoder produces them),
packed into pinned ring buffers, uploaded with hipMemcpyAsync on a copy stream while the previous batch computes,
and reduced to the grid-cell averaged flow (rows*cols (u,v) means per pair).  k-means over those vectors is then a
small streaming-Lloyd problem (cluster.KMeans).  With a model (fitted (k,2) centres) the stream also applies it: every
pair's field is labelled against the centres and counted per grid cell on the device while it is still there
(finish_clusters), so a fit can be deployed on footage that keeps arriving or is longer than memory.  With a histogram
(histogram=(bins, range)) every pair's field is also added to the stream's (u,v) table (uvhist.py), so a model can be fitted
on such footage too: histogram().fit(k).  With a camera (camera="affine") every pair's camera motion is fitted and subtracted
on the device straight after the flow (camera.py), and all of the above see the residual field.  With blobs
(blobs=dict(thr=...)) every pair's moving regions are labelled and described on the device as well (blobs.py): blobs();
with max_links among them the blobs of consecutive pairs are linked too, inside a batch and across batches (blobs.tracks).
With a photometric check (photometric=True or dict(tau=, kappa=, keep=)) every pair's vectors are checked against the batch's
own frames (photometric.py): photometric_stats(), and the blobs keep only the pixels that passed.
With a repair (repair=True or dict(radius=, rounds=, min_count=, smooth=, keep=)) the vectors that check flagged are filled
in by the median of their trusted neighbours before anything else looks at the field (repair.py): repair_stats().
With a forward-backward check (consistency=True or dict(alpha=, beta=, keep=)) every batch's flow is computed in both
directions from one front end and every pair's vectors are checked against the flow back (consistency.py):
consistency_stats(); the repair and the blobs use its states as they use the photometric check's.  One check per stream.
With trajectories (trajectories=True or dict(step=, seeds=, use_state=)) points are followed through the clip's repaired
fields, across batches (trajectories.py): trajectories() after a finish."""
import ctypes as C

import numpy as np

from ._lib import FbParams, check, load, ptr


class FlowStream:
    def __init__(self, W, H, batch_pairs=8, rows=14, cols=25, params=None, device=0, centers=None, mean=None, sums=False,
                 histogram=None, camera=None, blobs=None, photometric=None, repair=None, consistency=None, trajectories=None):
        self.W, self.H, self.rows, self.cols = W, H, rows, cols
        self.params = params or FbParams()
        h = C.c_void_p()
        check(load().ofc_stream_create(device, W, H, C.byref(self.params), batch_pairs, rows, cols, C.byref(h)))
        self._h = h
        self.pushed = 0
        self.k, self.sums = 0, False
        self.hist = None                    # (bins, range) of the stream's histogram, or None
        if centers is not None:
            self.set_model(centers, mean, sums)
        if histogram is not None:
            self.set_histogram(*histogram)
        self.camera = None                  # (model, thresholds) of the stream's camera, or None
        self._last_pairs = 0                # pairs the last finish delivered
        if camera is not None:
            self.set_camera(camera)
        self.blob_args = None               # (connectivity, thr, min_area, max_blobs) of the stream's blobs, or None
        self.max_links = 0                  # of the stream's blob links, 0 without them
        if blobs is not None:
            self.set_blobs(**blobs)
        self.photo_args = None              # (tau_q, kappa_q, keep) of the stream's photometric check, or None
        if photometric is not None and photometric is not False:
            self.set_photometric(**({} if photometric is True else photometric))
        self.consist_args = None            # (alpha_q, beta_q, keep) of the stream's forward-backward check, or None
        if consistency is not None and consistency is not False:
            self.set_consistency(**({} if consistency is True else consistency))
        self.repair_args = None             # (keep, radius, rounds, min_count, smooth) of the stream's repair, or None
        if repair is not None and repair is not False:
            self.set_repair(**({} if repair is True else repair))
        self.traj_points = 0                # the points the stream follows, 0 without trajectories
        if trajectories is not None and trajectories is not False:
            self.set_trajectories(**({} if trajectories is True else trajectories))

    def set_trajectories(self, step=8, seeds=None, use_state=False, on=True):
        """from the next clip on, follow points through every pair's field (ofc_stream_set_traj; trajectories.py has the
        definition): seeds int32 (P,2) in 1/65536 px, None for trajectories.grid_seeds(W, H, step).  The points are placed at
        the first pair after this call or after a finish and carried across batches; the advection runs directly behind the
        repair and before the moves and a camera, so a point lands by the whole flow.  use_state: a point ends where the state
        map of the stream's check is not in that check's keep; ValueError without a check.  on=False removes the stage.
        Only on a stream that holds no frame and no undelivered result, as set_model; ValueError otherwise."""
        if not on:
            check(load().ofc_stream_set_traj(self._h, 0, None, 0))
            self.traj_points, self._last_pairs = 0, 0
            return
        from .trajectories import _seeds
        s = _seeds(seeds, self.W, self.H, step)
        check(load().ofc_stream_set_traj(self._h, len(s), ptr(s), int(bool(use_state))))
        self.traj_points, self._last_pairs = len(s), 0

    def trajectories(self):
        """-> trajectories.Trajectories of the pairs the last finish() / finish_clusters() delivered (ofc_stream_read_traj); a
        point whose why is RAN was still live when the clip ended.  Straight after a finish only; ValueError once frames
        are held again, and on a stream without trajectories."""
        from .trajectories import Trajectories
        n, P = self._last_pairs, max(self.traj_points, 1)
        pos, length, why = np.zeros((max(n, 1) + 1, P, 2), np.int32), np.zeros(P, np.int32), np.zeros(P, np.uint8)
        check(load().ofc_stream_read_traj(self._h, ptr(pos), ptr(length), ptr(why), max(n, 1)))
        return Trajectories(pos[:n + 1], length, why)

    def set_consistency(self, alpha=None, beta=None, keep=(0,), on=True):
        """from the next batch on, compute every batch's flow in both directions from one front end
        (FlowEngine.calc_frames_dev_bidir) and put every pair's vectors to the forward-backward check (ofc_stream_set_consist;
        consistency.py has the definition), directly behind the flow and before the repair, the moves and a camera.  Its
        states then do what the photometric check's do: the repair fills what is not in `keep` (consistency.keep_mask), and
        on a stream with blobs those pixels belong to no blob.  A stream has one of the two checks: ValueError when the
        photometric one is on (and from set_photometric when this one is).  on=False removes it.  alpha and beta default to
        consistency.ALPHA and BETA.  Only on a stream that holds no frame and no undelivered result, as set_model;
        ValueError otherwise, and nothing changes."""
        if not on:
            check(load().ofc_stream_set_consist(self._h, 0, 0, 0, 0))
            self.consist_args, self._last_pairs = None, 0
            return
        from . import consistency as K
        args = K.quantise(K.ALPHA if alpha is None else alpha, K.BETA if beta is None else beta) + (K.keep_mask(keep),)
        check(load().ofc_stream_set_consist(self._h, 1, *args))
        self.consist_args, self._last_pairs = args, 0

    def consistency_stats(self):
        """-> (n, 4) int64 of the pairs the last finish() / finish_clusters() delivered (ofc_stream_read_consist): the pixels
        in each of the four states.  Straight after a finish only; ValueError once frames are held again, and on a stream
        without the check."""
        n = self._last_pairs
        counts = np.zeros((max(n, 1), 4), np.int64)
        check(load().ofc_stream_read_consist(self._h, ptr(counts), max(n, 1)))
        return counts[:n]

    def set_repair(self, radius=1, rounds=8, min_count=1, smooth=False, keep=(0,), on=True):
        """from the next batch on, repair every batch's field in place (ofc_stream_set_repair; repair.py has the definition)
        directly behind the photometric check, whose states say which vectors are sources (those in `keep`,
        consistency.keep_mask) and are updated: a filled pixel counts as CONSISTENT, so on a stream with blobs it belongs to
        them again.  Without a photometric check only vectors that are not usable numbers are filled.  It runs before the
        links' moves are taken and before a camera is fitted, so the cell means, the model's counts, the histogram, the
        camera and the blobs all see the repaired field.  on=False removes it.  rounds and min_count default to 8 and 1, a
        convention that is not tuned on anything here.  Only on a stream that holds no frame and no undelivered result, as
        set_model; ValueError otherwise, and nothing changes."""
        if not on:
            check(load().ofc_stream_set_repair(self._h, 0, 0, 0, 0, 0, 0))
            self.repair_args, self._last_pairs = None, 0
            return
        from .consistency import keep_mask
        args = (keep_mask(keep), int(radius), int(rounds), int(min_count), int(bool(smooth)))
        check(load().ofc_stream_set_repair(self._h, 1, *args))
        self.repair_args, self._last_pairs = args, 0

    def repair_stats(self):
        """-> (n, 3) int64 of the pairs the last finish() / finish_clusters() delivered (ofc_stream_read_repair): every pair's
        sources, filled and unfilled pixels.  Straight after a finish only; ValueError once frames are held again, and on a
        stream without the repair."""
        n = self._last_pairs
        counts = np.zeros((max(n, 1), 3), np.int64)
        check(load().ofc_stream_read_repair(self._h, ptr(counts), max(n, 1)))
        return counts[:n]

    def set_photometric(self, tau=8.0, kappa=0.5, keep=(0,), on=True):
        """from the next batch on, put every pair's vectors to the photometric check against the batch's own frames
        (ofc_stream_set_photo; photometric.py has the definition), directly behind the flow and before a camera is removed.
        On a stream with blobs the pixels whose state is not in `keep` (consistency.keep_mask) belong to no blob; the cell
        means, the model's counts, the histogram, the camera fit and the links' moves are left alone.  on=False removes the
        check.  tau and kappa default to 8 grey levels and 0.5, a convention that is not tuned on anything here.  Only on a
        stream that holds no frame and no undelivered result, as set_model; ValueError otherwise, and nothing changes."""
        if not on:
            check(load().ofc_stream_set_photo(self._h, 0, 0, 0, 0))
            self.photo_args, self._last_pairs = None, 0
            return
        from .photometric import keep_mask, quantise
        args = quantise(tau, kappa) + (keep_mask(keep),)
        check(load().ofc_stream_set_photo(self._h, 1, *args))
        self.photo_args, self._last_pairs = args, 0

    def photometric_stats(self):
        """-> (n, 5) int64 of the pairs the last finish() / finish_clusters() delivered (ofc_stream_read_photo): the pixels
        in each of the four states, then the sum of |e| in 1/256 grey levels over the compared ones; photometric.Photometric
        (None, stats, None, tau_q, kappa_q) gives the shares and the mean error.  Straight after a finish only; ValueError
        once frames are held again, and on a stream without the check."""
        n = self._last_pairs
        stats = np.zeros((max(n, 1), 5), np.int64)
        check(load().ofc_stream_read_photo(self._h, ptr(stats), max(n, 1)))
        return stats[:n]

    def set_blobs(self, thr=0.5, connectivity=8, min_area=1, max_blobs=4096, max_links=0):
        """from the next batch on, find every pair's moving objects (ofc_stream_set_blobs; blobs.py has the definition):
        foreground where the vector's length reaches thr (of the residual field, with a camera), keyed by the model's
        label where the stream has a model, so neighbouring regions of different motion stay apart; without one all keys
        are 0.  connectivity=None or 0 removes them.  max_links > 0 also links the blobs of consecutive pairs
        (ofc_stream_set_blob_links; blobs.link has the definition): across the pairs of a batch, across batches, by the
        moves of the field before the camera is removed; a finish ends the chain.  max_links=0 removes the links.  Only on
        a stream that holds no frame and no undelivered result, as set_model; ValueError otherwise, and nothing changes."""
        if not connectivity:
            check(load().ofc_stream_set_blobs(self._h, 0, 0.0, 1, 1))        # removes the links with them
            self.blob_args, self.max_links = None, 0
            return
        from .blobs import check_args, check_link_args
        args = (int(connectivity), float(thr), int(min_area), int(max_blobs))
        check_args(self.W, self.H, 1, args[0], args[2], args[3])             # both calls or neither: refuse before the first
        if max_links:
            check_link_args(self.W, self.H, 1, args[2], max_links)
        check(load().ofc_stream_set_blobs(self._h, *args))
        self.blob_args = args
        self._last_pairs = 0
        check(load().ofc_stream_set_blob_links(self._h, int(max_links)))
        self.max_links = int(max_links)

    def blobs(self):
        """-> blobs.Blobs (records and found; no label map) of the pairs the last finish() / finish_clusters() delivered
        (ofc_stream_read_blobs).  Straight after a finish only; ValueError once frames are held again, and on a stream
        without blobs.  With max_links it carries links and nlinks (ofc_stream_read_blob_links) for blobs.tracks."""
        from .blobs import LINK_NF, NF, Blobs, _split_links, order_records
        n, mb = self._last_pairs, self.blob_args[3] if self.blob_args else 1
        table = np.zeros((max(n, 1), mb, NF), np.int64)
        cnt, found = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        check(load().ofc_stream_read_blobs(self._h, ptr(table), ptr(cnt), ptr(found), max(n, 1)))
        out = Blobs(self.W, self.H, None, [order_records(table[i, :cnt[i]], int(cnt[i]), mb) for i in range(n)], found[:n])
        if self.max_links:
            nt = max(n - 1, 0)
            links, nlinks = np.zeros((max(nt, 1), self.max_links, LINK_NF), np.int64), np.zeros(max(nt, 1), np.int32)
            check(load().ofc_stream_read_blob_links(self._h, ptr(links), ptr(nlinks), max(nt, 1)))
            out.links, out.nlinks = _split_links(links[:nt], nlinks[:nt]), nlinks[:nt]
        return out

    def set_camera(self, camera, thresholds=None):
        """from the next batch on, fit every pair's camera motion and subtract it in place before anything else looks at
        the field (ofc_stream_set_camera): the cell means, the model's counts and the histogram then see the residual.
        camera: None (removes it), 'translation', 'affine' or (kind, thresholds); thresholds as camera.compensate's (the
        default (4.0, 2.0, 1.0) is a guess, not tuned on any footage).  Only on a stream that holds no frame and no
        undelivered result, as set_model; ValueError otherwise, and nothing changes."""
        from .camera import camera_args, parse_camera
        if thresholds is not None and isinstance(camera, str):
            camera = (camera, thresholds)
        cam = parse_camera(camera)
        if cam is None:
            check(load().ofc_stream_set_camera(self._h, 0, None, 0))
        else:
            kind, thr, T = camera_args(*cam)
            check(load().ofc_stream_set_camera(self._h, kind, ptr(thr), T))
        self.camera = cam
        self._last_pairs = 0

    def camera_motion(self):
        """-> camera.CameraMotion of the pairs the last finish() / finish_clusters() delivered (ofc_stream_read_camera):
        params (n,6) and status (n,); the stream keeps no moments, so inliers and outside are None.  Straight after a
        finish only; ValueError once frames are held again, and on a stream without a camera."""
        from .camera import CameraMotion
        n = self._last_pairs
        params, status = np.zeros((max(n, 1), 6)), np.zeros(max(n, 1), np.int32)
        check(load().ofc_stream_read_camera(self._h, ptr(params), ptr(status), max(n, 1)))
        return CameraMotion(params[:n], status[:n], None, None)

    def set_histogram(self, bins, range=32.0):
        """from the next batch on, add every pair's field to the stream's (u,v) histogram (ofc_stream_set_histogram, the
        kernel of uvhist.uv_histogram); bins=None or 0 removes it.  Only on a stream that holds no frame and no undelivered
        result, as set_model; ValueError otherwise, and nothing changes.  The same (bins, range) again keeps the table."""
        if not bins:
            check(load().ofc_stream_set_histogram(self._h, 0, 0.0))
            self.hist = None
            return
        from .uvhist import check_params
        bins, range = check_params(bins, range)
        check(load().ofc_stream_set_histogram(self._h, bins, range))
        self.hist = (bins, range)

    def histogram(self, reset=True):
        """-> uvhist.UVHistogram of every pair since the table was last reset (ofc_stream_read_histogram); with reset the
        table then starts over, without it the next clips add to it.  Straight after finish() / finish_clusters() only (or on
        a fresh stream: an empty table); ValueError otherwise, and on a stream without a histogram."""
        from .uvhist import UVHistogram, table_len
        table = np.empty(table_len(self.hist[0]) if self.hist else 1, np.int64)
        check(load().ofc_stream_read_histogram(self._h, ptr(table), int(bool(reset))))
        return UVHistogram(self.hist[0], self.hist[1], table)

    def set_model(self, centers, mean=None, sums=False):
        """from the next batch on, label every pair's field against `centers` ((k,2), un-centred; None removes the model)
        and count it per cell (ofc_stream_set_model, the kernel of vis.grid_assign_counts).  Only on a stream that holds
        no frame and no undelivered result: fresh, or straight after finish() / finish_clusters(); ValueError otherwise,
        and the model stays as it was.
        mean=None labels against mean (0, 0), KMeans.predict's un-centred E-step: a stream has no field mean before the
        clip ends.  ClipPipeline.assign centres by the field's mean; the two agree except where a pixel's two nearest
        centres tie to the rounding of the expanded form, so no bit equality between the two routes is promised."""
        if centers is None:
            check(load().ofc_stream_set_model(self._h, 0, None, None, 0))
            self.k, self.sums = 0, False
            return
        from .vis import _model_args
        k, mean, cen_c = _model_args(centers, mean)
        check(load().ofc_stream_set_model(self._h, k, ptr(mean), ptr(cen_c), int(bool(sums))))
        self.k, self.sums = k, bool(sums)

    def push(self, gray):
        gray = np.ascontiguousarray(gray, np.uint8)
        if gray.shape != (self.H, self.W):
            raise ValueError(f"expected a {self.H}x{self.W} uint8 frame")
        done = C.c_int()
        check(load().ofc_stream_push_gray(self._h, ptr(gray), C.byref(done)))
        self.pushed += 1
        return done.value

    def finish(self):
        """-> cell_uv (n_pairs, rows*cols, 2) float32"""
        n = max(self.pushed - 1, 0)
        out = np.empty((max(n, 1), self.rows * self.cols, 2), np.float32)
        got = C.c_int()
        check(load().ofc_stream_finish(self._h, ptr(out), max(n, 1), C.byref(got)))
        self.pushed = 0
        self._last_pairs = got.value
        return out[:got.value]

    def finish_clusters(self):
        """finish() that also delivers what the model says: -> (cell_uv, counts (n_pairs, rows*cols, k) int32), and with
        a model set with sums=True also sums (n_pairs, rows*cols, k, 2) f64.  ValueError without a model."""
        n = max(self.pushed - 1, 0)
        cells, k = self.rows * self.cols, max(self.k, 1)
        out = np.empty((max(n, 1), cells, 2), np.float32)
        counts = np.empty((max(n, 1), cells, k), np.int32)
        sums = np.empty((max(n, 1), cells, k, 2), np.float64) if self.sums else None
        got = C.c_int()
        check(load().ofc_stream_finish_clusters(self._h, ptr(out), ptr(counts), ptr(sums), max(n, 1), C.byref(got)))
        self.pushed = 0
        self._last_pairs = got.value
        res = (out[:got.value], counts[:got.value])
        return res + (sums[:got.value],) if self.sums else res

    def close(self):
        if getattr(self, "_h", None):
            load().ofc_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def grid_cell_mean_flow(flow, rows=14, cols=25, device=0):
    flow = np.ascontiguousarray(flow, np.float32)
    H, W = flow.shape[:2]
    out = np.empty((rows * cols, 2), np.float32)
    check(load().ofc_grid_cell_mean_flow(device, ptr(flow), W, H, rows, cols, ptr(out)))
    return out
