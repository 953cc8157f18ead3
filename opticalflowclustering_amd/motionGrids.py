"""The clip-wide motion fit as a table: one row per frame pair, one value per cell of the 14 x 25 grid, in the format of
KmeanGrids.process_video's hue CSV (which findCosineDifferentVectors.py compares column by column).

A clip's (u,v) vectors are clustered over the whole clip (ClipPipeline.run_kmeans), or labelled against the centres of
another clip's fit (ClipPipeline.assign), and ClipPipeline.cell_clusters() counts on the device how many pixels of every
cell fall into every cluster.  A cell's value is its dominant cluster, written as the hue the reference's colour coding
gives that cluster's direction (computeOpticalFlowModule.py:25-33: hue = angle / 2), or as the cluster index.

    python -m opticalflowclustering_amd.motionGrids --path CLIP -c 5 -f OUT.csv --save-model centres.npy
    python -m opticalflowclustering_amd.motionGrids --path OTHER -c 5 -f OTHER.csv --model centres.npy
    python -m opticalflowclustering_amd.motionGrids --path LONG -c 5 -f LONG.csv --model centres.npy --stream
    python -m opticalflowclustering_amd.motionGrids --path LONG -c 5 -f LONG.csv --fit-stream --n-init 4

With --stream the clip is never resident: its frames are read one at a time and pushed through a FlowStream that carries
the model, which labels and counts every batch's field on the device while it is there (FlowStream.finish_clusters), so
the clip may be longer than memory.  A stream has no field mean before it ends: it labels against mean (0, 0), as
KMeans.predict does, where ClipPipeline.assign centres the arithmetic by the field's mean.  The two agree except where a
pixel's two nearest centres tie to the rounding of the expanded form; bit equality of the two routes is not promised.

With --fit-stream the clip is never resident either, and the model is fitted on it all the same, in two passes over the
file.  Pass 1 pushes the frames through a FlowStream that adds every pair's field to a (u,v) histogram (uvhist.py) and fits
the centres on that table (-c, --seed, an --init file and --n-init restarts apply); pass 2 is the --stream route with those
centres.  Vectors outside --hist-range take no part in the fit; their share is printed.

With --camera translation|affine every pair's camera motion is fitted and removed on the device before anything else looks at
the field (camera.py), on the resident route, on --stream and on --fit-stream: the clusters then describe the scene and not
the camera, and --weights moving:0.5 means "moves against the background".  --camera-out writes the (pairs, 6) models.

With --blobs FILE.csv every pair's moving objects are found on the device as well (blobs.py) and written one row per blob:
pair, key, root x, root y, area, box, centroid, mean u, mean v.  A pixel is foreground when its vector's length reaches
--blob-thr, and is keyed by its label against the centres (un-centred, as a stream labels), so neighbouring regions of
different motion are different blobs; --blob-min-area drops small ones, --blob-connectivity is 4 or 8.  The same rows come
out of the resident route, --stream and --fit-stream, with --camera after the camera is removed.
With --tracks (it needs --blobs) the blobs of consecutive pairs are linked on the device as well (blobs.link: a blob's pixels
land, by their own flow vectors before the camera is removed, on the next pair's blobs) and every row gets a last column,
the id of the track its blob belongs to (blobs.tracks).

With --consistent (resident route only) the flow is computed a second time over the reversed clip and every vector is put
to the forward-backward check on the device (consistency.py), before any camera removal: the fit then gives weight 0 to
every pixel that failed it, and the --blobs key map keeps only those that passed.  --fb-alpha and --fb-beta are the check's
two constants (the literature's 0.01 and 0.5 px^2 by default, not tuned here); --fb-counts writes the (pairs, 4) pixel
counts per state.

With --trajectories FILE.npz a grid of points (--traj-step px apart) is followed through the clip's fields (trajectories.py),
behind the repair and before the camera is removed, on the resident route, on --stream and on --fit-stream; pos, length and
why go to FILE.npz.
With --photometric every vector is put to the photometric check instead (photometric.py): the next frame, read where the
pixel lands, must show the pixel's own grey value to within --photo-tau grey levels plus --photo-kappa times the local
contrast (8 and 0.5 by default, a convention that is not tuned here).  It needs no second flow, so it works on the resident
route, where it does what --consistent does with its state map, and on --stream and --fit-stream, where the stream's blobs
keep only the pixels that passed.  --photo-counts writes the (pairs, 5) stats: the pixels per state, then the sum of the
absolute error in 1/256 grey levels.  The two checks cannot be combined.

With --repair R[:ROUNDS] (any route) the vectors that are not trusted are filled in on the device before anything else looks
at the field (repair.py): each becomes the median of the trusted vectors in its (2R+1)^2 window, R being 1 or 2, round after
round, ROUNDS times at the most (8 by default, a convention that is not tuned here).  With --consistent or --photometric the
vectors that failed the check are the ones filled, and a filled pixel counts as one that passed; without a check only vectors
that are not usable numbers are.  --repair-smooth adds a median pass over the whole field; --repair-counts writes the
(pairs, 3) counts: sources, filled, unfilled.
"""
import argparse
import os

import numpy as np


def dominant(counts):
    """the cluster with the most pixels per cell: the first maximum, so ties (an empty cell included) go to the lowest
    cluster index.  counts (..., k) -> (...)"""
    return np.argmax(np.asarray(counts), axis=-1)


def centre_hues(centers):
    """the hue (0..179) flow_to_bgr paints a centre's direction with: its angle in degrees, halved and truncated.
    (0, 0) has angle 0; an angle that rounds up to 360 wraps to hue 0.  centers (k,2) -> (k,) int64"""
    cen = np.asarray(centers, np.float64).reshape(-1, 2)
    return np.array([int(np.degrees(np.arctan2(v, u)) % 360.0 / 2.0) % 180 for u, v in cen], np.int64)


def hue_rows(counts, centers):
    """counts (n, cells, k), centers (k,2) -> (n, cells) int64: the hue of every cell's dominant cluster"""
    counts = np.asarray(counts)
    hues = centre_hues(centers)
    if counts.shape[-1] != len(hues):
        raise ValueError(f"counts are over {counts.shape[-1]} clusters, centers has {len(hues)}")
    return hues[dominant(counts)]


def write_csv(path, rows):
    """header cell_0 .. cell_{n-1}, then one comma-separated line of integers per row (KmeanGrids.py:394-399)"""
    rows = np.asarray(rows)
    if rows.ndim != 2:
        raise ValueError(f"rows must be (n, cells), got shape {rows.shape}")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w", newline="") as f:
        f.write(",".join(f"cell_{i}" for i in range(rows.shape[1])) + "\n")
        for r in rows:
            f.write(",".join(str(int(h)) for h in r) + "\n")


MAX_BLOBS = 4096            # per pair; a pair with more delivers none (blobs.py), and its row count says so
MAX_LINKS = 4096            # per transition, with --tracks; a transition with more delivers none and breaks every track


def write_blob_csv(path, blobs, tracks=False):
    """blobs.CSV_HEADER, then one line per blob (blobs.Blobs.rows()), pairs in order and a pair's blobs by root; with
    tracks (the Blobs then carries links) blobs.TRACK_CSV_HEADER and the track id as a last column"""
    from .blobs import CSV_HEADER, TRACK_CSV_HEADER
    from .blobs import tracks as find_tracks
    found = find_tracks(blobs) if tracks else None
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w", newline="") as f:
        f.write(",".join(TRACK_CSV_HEADER if tracks else CSV_HEADER) + "\n")
        for r in blobs.rows(found):
            f.write(",".join(str(v) for v in r) + "\n")
    if found is not None and found.broken:
        print(f"tracks: {len(found.broken)} transition(s) broke every track through them (first: {found.broken[0]})")
    over = [i for i, n in enumerate(blobs.found) if n > MAX_BLOBS]
    if over:
        print(f"blobs: {len(over)} pair(s) hold more than {MAX_BLOBS} components and deliver none (first: pair {over[0]})")


def parse_weights(text):
    """'none' -> None, 'magnitude' -> 'magnitude', 'moving:THR' -> ('moving', THR): ClipPipeline's sample_weight"""
    if text == "none":
        return None
    if text == "magnitude":
        return "magnitude"
    kind, _, thr = text.partition(":")
    if kind == "moving" and thr:
        try:
            return ("moving", float(thr))
        except ValueError:
            pass
    raise argparse.ArgumentTypeError(f"weights should be none, magnitude or moving:THR, got {text!r}")


def parse_thresholds(text):
    """'4,2,1' -> (4.0, 2.0, 1.0); '' -> (): the --camera-thresholds, finite and positive, at most eight"""
    try:
        thr = tuple(float(t) for t in text.split(",") if t.strip())
    except ValueError:
        thr = None
    if thr is None or len(thr) > 8 or not all(np.isfinite(t) and t > 0 for t in thr):
        raise argparse.ArgumentTypeError(f"thresholds should be up to eight positive numbers like 4,2,1, got {text!r}")
    return thr


def parse_arguments(argv=None):
    ap = argparse.ArgumentParser(prog="python -m opticalflowclustering_amd.motionGrids", description=__doc__.split("\n\n")[0])
    ap.add_argument("--path", required=True, help="input video (.npy/.npz stack, image directory, or a video with cv2)")
    ap.add_argument("-c", "--clusters", required=True, type=int, help="number of motion clusters")
    ap.add_argument("-f", "--csv", required=True, help="output table: one row per frame pair, one column per cell")
    ap.add_argument("--rows", type=int, default=14)
    ap.add_argument("--cols", type=int, default=25)
    ap.add_argument("--init", default="k-means++", help="k-means++ or a .npy file with (k,2) initial centres")
    ap.add_argument("--seed", type=int, default=0, help="random_state of the k-means++ seeding")
    ap.add_argument("--weights", type=parse_weights, default=None, metavar="none|magnitude|moving:THR",
                    help="sample weights of the fit")
    ap.add_argument("--model", help=".npy file with (k,2) centres: label against them instead of fitting")
    ap.add_argument("--save-model", help="write the centres used (fitted or given) to this .npy file")
    ap.add_argument("--counts", help="write the (pairs, cells, k) pixel counts to this .npy file")
    ap.add_argument("--value", choices=("hue", "label"), default="hue",
                    help="a cell's value: the hue of its dominant cluster's direction, or that cluster's index")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--stream", action="store_true",
                    help="with --model: read the clip frame by frame and count on a FlowStream; the clip is never resident")
    ap.add_argument("--batch-pairs", type=int, default=8, help="frame pairs per batch of the --stream route")
    ap.add_argument("--fit-stream", action="store_true",
                    help="fit on the clip's (u,v) histogram, built on a FlowStream, then count as --stream does: two passes "
                         "over the file, the clip is never resident")
    ap.add_argument("--hist-bins", type=int, default=1024, help="bins per axis of the --fit-stream histogram (a power of two)")
    ap.add_argument("--hist-range", type=float, default=32.0,
                    help="the --fit-stream histogram covers [-RANGE, RANGE) px on both axes (a power of two)")
    ap.add_argument("--n-init", type=int, default=1, help="k-means++ restarts of the --fit-stream fit; the lowest inertia wins")
    ap.add_argument("--camera", choices=("none", "translation", "affine"), default="none",
                    help="fit and remove every pair's camera motion before anything else looks at the field")
    ap.add_argument("--camera-thresholds", type=parse_thresholds, default=(4.0, 2.0, 1.0), metavar="4,2,1",
                    help="inlier radii in px of the camera fit's re-selection rounds (the default is a guess, not tuned)")
    ap.add_argument("--camera-out", metavar="FILE.npy", help="write the (pairs, 6) camera models to this .npy file")
    ap.add_argument("--blobs", metavar="FILE.csv", help="write one row per moving object (connected component) to this file")
    ap.add_argument("--blob-thr", type=float, default=0.5, help="a pixel is foreground when its vector's length reaches this, px")
    ap.add_argument("--blob-min-area", type=int, default=1, help="smallest component, in pixels, that becomes a row")
    ap.add_argument("--blob-connectivity", type=int, choices=(4, 8), default=8)
    ap.add_argument("--tracks", action="store_true",
                    help="link the blobs of consecutive pairs and add a track id as the last column of the --blobs file")
    ap.add_argument("--consistent", action="store_true",
                    help="forward-backward check of every vector (resident route): failed pixels get weight 0 and no blob")
    ap.add_argument("--fb-alpha", type=float, default=0.01, help="relative term of the check (a convention, not tuned)")
    ap.add_argument("--fb-beta", type=float, default=0.5, help="absolute term of the check in px^2 (a convention, not tuned)")
    ap.add_argument("--fb-counts", metavar="FILE.npy", help="write the (pairs, 4) pixel counts per state to this .npy file")
    ap.add_argument("--photometric", action="store_true",
                    help="photometric check of every vector against the frames (any route): failed pixels get weight 0 on the "
                         "resident route and no blob on every route")
    ap.add_argument("--photo-tau", type=float, default=8.0, help="absolute term of the check in grey levels (a convention, not tuned)")
    ap.add_argument("--photo-kappa", type=float, default=0.5,
                    help="grey levels forgiven per grey level of local contrast (a convention, not tuned)")
    ap.add_argument("--photo-counts", metavar="FILE.npy", help="write the (pairs, 5) stats of the check to this .npy file")
    ap.add_argument("--repair", metavar="R[:ROUNDS]",
                    help="fill the vectors that are not trusted by the median of their (2R+1)^2 window, R = 1 or 2, for at most "
                         "ROUNDS rounds (default 8, a convention, not tuned); any route")
    ap.add_argument("--repair-smooth", action="store_true", help="a median pass over the whole field behind the fill")
    ap.add_argument("--repair-counts", metavar="FILE.npy", help="write the (pairs, 3) counts of the repair to this .npy file")
    ap.add_argument("--trajectories", metavar="FILE.npz",
                    help="follow a grid of points through the clip's (repaired) fields and write pos, length and why to this "
                         ".npz file (any route)")
    ap.add_argument("--traj-step", type=float, default=8.0, help="spacing of the seed grid in px (default 8)")
    args = ap.parse_args(argv)
    if not (np.isfinite(args.traj_step) and args.traj_step > 0):
        ap.error("--traj-step must be a positive number of pixels")
    if args.traj_step != 8.0 and not args.trajectories:
        ap.error("--traj-step belongs to --trajectories")
    args.traj_spec = dict(step=args.traj_step) if args.trajectories else None
    args.repair_spec = None
    if args.repair:
        try:
            parts = [int(v) for v in args.repair.split(":")]
            if len(parts) > 2:
                raise ValueError
        except ValueError:
            ap.error(f"--repair takes R or R:ROUNDS, two integers, got {args.repair!r}")
        radius, rounds = parts[0], parts[1] if len(parts) == 2 else 8
        if radius not in (1, 2) or not 0 <= rounds <= 254 or (rounds == 0 and not args.repair_smooth):
            ap.error("--repair R[:ROUNDS]: R is 1 or 2, ROUNDS 0 .. 254, and 0 only with --repair-smooth")
        args.repair_spec = dict(radius=radius, rounds=rounds, smooth=args.repair_smooth)
    elif args.repair_smooth or args.repair_counts:
        ap.error("--repair-smooth and --repair-counts belong to --repair")
    if args.photometric:
        if args.consistent:
            ap.error("--photometric and --consistent each leave a state map of their own: combining the two is not supported")
        from .photometric import quantise as photo_quantise
        try:
            photo_quantise(args.photo_tau, args.photo_kappa)
        except ValueError as e:
            ap.error(str(e))
    elif args.photo_counts or args.photo_tau != 8.0 or args.photo_kappa != 0.5:
        ap.error("--photo-tau, --photo-kappa and --photo-counts belong to --photometric")
    args.photo_spec = dict(tau=args.photo_tau, kappa=args.photo_kappa) if args.photometric else None
    if args.consistent:
        for flag, given in (("--stream", args.stream), ("--fit-stream", args.fit_stream)):
            if given:
                ap.error(f"--consistent needs the resident clip (a stream would need the engine a second time): not with {flag}")
        from .consistency import quantise
        try:
            quantise(args.fb_alpha, args.fb_beta)
        except ValueError as e:
            ap.error(str(e))
    elif args.fb_counts or args.fb_alpha != 0.01 or args.fb_beta != 0.5:
        ap.error("--fb-alpha, --fb-beta and --fb-counts belong to --consistent")
    if args.camera_out and args.camera == "none":
        ap.error("--camera-out needs --camera translation or --camera affine")
    args.camera_spec = None if args.camera == "none" else (args.camera, args.camera_thresholds)
    if not (np.isfinite(args.blob_thr) and args.blob_thr >= 0):
        ap.error("--blob-thr must be finite and >= 0")
    if args.blob_min_area < 1:
        ap.error("--blob-min-area must be at least 1")
    args.blob_spec = dict(thr=args.blob_thr, connectivity=args.blob_connectivity, min_area=args.blob_min_area,
                          max_blobs=MAX_BLOBS) if args.blobs else None
    if args.tracks and not args.blobs:
        ap.error("--tracks adds a column to the --blobs file: it needs --blobs FILE.csv")
    args.max_links = MAX_LINKS if args.tracks else 0
    if args.fit_stream:
        for flag, given in (("--model", args.model), ("--stream", args.stream), ("--weights", args.weights)):
            if given:
                ap.error(f"--fit-stream fits its own model on an unweighted stream: it cannot be combined with {flag}")
        from .uvhist import check_params
        try:
            check_params(args.hist_bins, args.hist_range)
        except ValueError as e:
            ap.error(str(e))
        if args.n_init < 1:
            ap.error("--n-init must be at least 1")
    if args.stream and not args.model:
        ap.error("--stream applies a model to arriving frames and cannot fit one: it requires --model")
    if args.batch_pairs < 1:
        ap.error("--batch-pairs must be at least 1")
    return args


def _load_centres(path, k, what):
    cen = np.asarray(np.load(path), np.float64)
    if cen.shape != (k, 2):
        raise ValueError(f"{what} {path!r} holds an array of shape {cen.shape}, expected ({k}, 2)")
    return cen


def gray_frames(path, device=0):
    """the clip's frames one at a time as (H, W) u8 grey (cv2's BGR2GRAY, on the device, for three-channel frames)"""
    from .frameio import FrameSource
    from .vis import bgr2gray
    cap = FrameSource(path)
    try:
        while cap.isOpened():
            ret, frame = cap.read()
            if not ret:
                break
            yield bgr2gray(frame, device) if frame.ndim == 3 else np.ascontiguousarray(frame, np.uint8)
    finally:
        cap.release()


def read_gray_frames(path, device=0):
    """every frame of the clip as (T, H, W) u8 grey (cv2's BGR2GRAY, on the device, for three-channel frames)"""
    frames = list(gray_frames(path, device))
    if len(frames) < 2:
        raise RuntimeError(f"{path!r} has {len(frames)} frame(s); a flow field needs two")
    return np.stack(frames)


def _save_npy(path, a):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    np.save(path, a)


def _save_trajectories(path, tr):
    """pos (pairs+1, P, 2) int32 in 1/65536 px, length (P,) int32 and why (P,) u8 as one .npz archive under exactly this name"""
    from .trajectories import WHY_NAMES
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "wb") as f:
        np.savez(f, pos=tr.pos, length=tr.length, why=tr.why)
    ends = np.bincount(tr.why, minlength=4)
    print(f"trajectories: {len(tr)} points over {tr.n_pairs} pairs, " + ", ".join(f"{int(c)} {name}" for name, c in zip(WHY_NAMES, ends)))


def _print_repair(counts):
    total = max(int(counts.sum()), 1)
    print("repair: " + ", ".join(f"{100.0 * c / total:.2f} % {name}" for name, c in zip(("sources", "filled", "unfilled"), counts.sum(0))))


def _print_photometric(stats, tau_q, kappa_q):
    from .photometric import STATE_NAMES, Photometric
    ph = Photometric(None, stats, None, tau_q, kappa_q)
    total, compared = ph.counts.sum(), ph.counts[:, :2].sum()
    print("photometric check: " + ", ".join(f"{100.0 * s:.2f} % {name}" for name, s in zip(STATE_NAMES, ph.counts.sum(0) / max(total, 1)))
          + (f"; mean absolute error {ph.abs_error.sum() / (256.0 * compared):.3f} grey levels" if compared else ""))


def stream_counts(path, centers, rows, cols, batch_pairs=8, device=0, camera=None, camera_out=None, blobs=None, blobs_out=None,
                  max_links=0, photometric=None, photo_out=None, repair=None, repair_out=None, trajectories=None, traj_out=None):
    """the (pairs, cells, k) counts of a model on a clip that is read frame by frame and never resident; camera as
    FlowStream's, its (pairs, 6) models saved to camera_out; blobs as FlowStream's, their rows written to blobs_out, with
    max_links linked and with their track ids; photometric as FlowStream's, its (pairs, 5) stats saved to photo_out; repair
    as FlowStream's, its (pairs, 3) counts saved to repair_out; trajectories as FlowStream's, saved to traj_out"""
    from .stream import FlowStream
    fs, n = None, 0
    if blobs is not None and max_links:
        blobs = dict(blobs, max_links=max_links)
    try:
        for gray in gray_frames(path, device):
            if fs is None:
                fs = FlowStream(gray.shape[1], gray.shape[0], batch_pairs, rows, cols, device=device, centers=centers,
                                camera=camera, blobs=blobs, photometric=photometric, repair=repair,
                                trajectories=trajectories if traj_out else None)
            fs.push(gray)
            n += 1
        if n < 2:
            raise RuntimeError(f"{path!r} has {n} frame(s); a flow field needs two")
        counts = fs.finish_clusters()[1]
        if camera is not None and camera_out:
            np.save(camera_out, fs.camera_motion().params)
        if blobs is not None and blobs_out:
            write_blob_csv(blobs_out, fs.blobs(), tracks=bool(max_links))
        if photometric is not None:
            stats = fs.photometric_stats()
            _print_photometric(stats, *fs.photo_args[:2])
            if photo_out:
                _save_npy(photo_out, stats)
        if repair is not None:
            filled = fs.repair_stats()
            _print_repair(filled)
            if repair_out:
                _save_npy(repair_out, filled)
        if trajectories is not None and traj_out:
            _save_trajectories(traj_out, fs.trajectories())
        return counts
    finally:
        if fs is not None:
            fs.close()


def stream_histogram(path, bins, range, rows=14, cols=25, batch_pairs=8, device=0, camera=None, photometric=None, repair=None):
    """the (u,v) histogram (uvhist.UVHistogram) of a clip that is read frame by frame and never resident; with repair (and the
    photometric check that says what to repair) as FlowStream's, of the repaired field"""
    from .stream import FlowStream
    fs, n = None, 0
    try:
        for gray in gray_frames(path, device):
            if fs is None:
                fs = FlowStream(gray.shape[1], gray.shape[0], batch_pairs, rows, cols, device=device, histogram=(bins, range),
                                camera=camera, photometric=photometric if repair is not None else None, repair=repair)
            fs.push(gray)
            n += 1
        if n < 2:
            raise RuntimeError(f"{path!r} has {n} frame(s); a flow field needs two")
        fs.finish()
        return fs.histogram()
    finally:
        if fs is not None:
            fs.close()


def main(argv=None):
    args = parse_arguments(argv)
    k = args.clusters
    given = _load_centres(args.model, k, "--model") if args.model else \
        _load_centres(args.init, k, "--init") if args.init != "k-means++" else None
    if args.fit_stream:
        hist = stream_histogram(args.path, args.hist_bins, args.hist_range, args.rows, args.cols, args.batch_pairs, args.device,
                                args.camera_spec, args.photo_spec, args.repair_spec)
        total = hist.n + hist.outside
        print(f"histogram: {hist.n} vectors in {int(np.count_nonzero(hist.counts))} bins, {hist.outside} outside "
              f"[-{args.hist_range:g}, {args.hist_range:g}) px ({100.0 * hist.outside / max(total, 1):.4f} %)")
        centers, _, _ = hist.fit(k, init="k-means++" if given is None else given, random_state=args.seed, n_init=args.n_init,
                                 device=args.device)
        counts = stream_counts(args.path, centers, args.rows, args.cols, args.batch_pairs, args.device, args.camera_spec,
                               args.camera_out, args.blob_spec, args.blobs, args.max_links, args.photo_spec, args.photo_counts,
                               args.repair_spec, args.repair_counts, args.traj_spec, args.trajectories)
        return _write_outputs(args, counts, centers)
    if args.stream:
        centers = given
        counts = stream_counts(args.path, centers, args.rows, args.cols, args.batch_pairs, args.device, args.camera_spec,
                               args.camera_out, args.blob_spec, args.blobs, args.max_links, args.photo_spec, args.photo_counts,
                               args.repair_spec, args.repair_counts, args.traj_spec, args.trajectories)
        return _write_outputs(args, counts, centers)
    from .pipeline import ClipPipeline
    frames = read_gray_frames(args.path, args.device)
    T, H, W = frames.shape
    pipe = ClipPipeline(W, H, T, device=args.device)
    try:
        pipe.upload_frames(frames)
        pipe.run_flow()
        fb = args.consistent
        if fb:                                  # before the camera is taken out: a residual does not say where a pixel lands
            from .consistency import STATE_NAMES
            pipe.run_backward_flow()
            checked = pipe.consistency(args.fb_alpha, args.fb_beta)
            print("forward-backward check: " + ", ".join(f"{100.0 * s:.2f} % {name}" for name, s in
                                                         zip(STATE_NAMES, checked.counts.sum(0) / max(checked.counts.sum(), 1))))
            if args.fb_counts:
                os.makedirs(os.path.dirname(args.fb_counts) or ".", exist_ok=True)
                np.save(args.fb_counts, checked.counts)
        if args.photo_spec:                     # like the other check: before the camera is taken out
            checked = pipe.photometric(**args.photo_spec)
            _print_photometric(checked.stats, checked.tau_q, checked.kappa_q)
            if args.photo_counts:
                _save_npy(args.photo_counts, checked.stats)
            fb = True
        if args.repair_spec:                    # a repaired vector says where a pixel lands: before the camera is taken out
            filled = pipe.repair(need_state=False, **args.repair_spec)
            _print_repair(filled)
            if args.repair_counts:
                _save_npy(args.repair_counts, filled)
        if args.traj_spec:                      # a point lands by the whole flow: before the camera is taken out
            _save_trajectories(args.trajectories, pipe.trajectories(**args.traj_spec))
        if args.camera_spec:
            if args.max_links:
                pipe.capture_moves()            # where the pixels go: before the camera is taken out of the field
            motion = pipe.compensate_camera(*args.camera_spec)
            if args.camera_out:
                np.save(args.camera_out, motion.params)
        if args.model:
            centers = given
            pipe.assign(centers)
        elif given is not None:
            centers, _, _ = pipe.run_kmeans(given, sample_weight=args.weights, consistent=fb)
        elif args.weights is not None or fb:    # sklearn's weighted k-means++ fit in its two-step form
            C0, _ = pipe.seed_kmeans(k, args.seed, sample_weight=args.weights, consistent=fb)
            centers, _, _ = pipe.run_kmeans(C0, sample_weight=args.weights, consistent=fb)
        else:
            centers, _, _ = pipe.run_kmeans("k-means++", k=k, random_state=args.seed)
        counts = pipe.cell_clusters(args.rows, args.cols)
        if args.blob_spec:
            write_blob_csv(args.blobs, pipe.blobs(by=centers, mean=None, labels=False, links=args.max_links or None,
                                                  consistent=fb, **args.blob_spec),
                           tracks=bool(args.max_links))
    finally:
        pipe.close()
    return _write_outputs(args, counts, centers)


def _write_outputs(args, counts, centers):
    write_csv(args.csv, hue_rows(counts, centers) if args.value == "hue" else dominant(counts))
    if args.save_model:
        np.save(args.save_model, centers)
    if args.counts:
        np.save(args.counts, counts)
    return counts, centers


if __name__ == "__main__":
    main()
