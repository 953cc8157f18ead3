"""Moving objects: connected components of a per-pixel key map, one integer record per component (csrc/blobs.hip;
include/ofc.h has the definition).  This stands where the reference read YOLO boxes and segmented contours from files
(KmeanGrids.py:16-50): after camera compensation "this pixel moves against the background" is a foreground test, a cluster
label is an identity, and grouping such pixels into regions says how many things move in a pair, where, how big, which way.

A key map is u8, 255 = background; two neighbouring pixels (connectivity 4: by an edge, 8: by an edge or a corner) belong to
one component iff their keys are equal and not 255.  A component is named by its root, its smallest y*W + x.  Everything
that comes back is an integer and does not depend on the order the device worked in."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DeviceBuffer, check, load, ptr

NF = _lib.BLOB_FIELDS
FIELDS = ("root", "key", "area", "xmin", "ymin", "xmax", "ymax", "sx", "sy", "nvalid", "squ", "sqv")
BACKGROUND = 255
CSV_HEADER = ("pair", "key", "root_x", "root_y", "area", "xmin", "ymin", "xmax", "ymax", "cx", "cy", "mean_u", "mean_v")
TRACK_CSV_HEADER = CSV_HEADER + ("track",)
LINK_NF = _lib.BLOB_LINK_FIELDS
LINK_FIELDS = ("root_a", "root_b", "votes")
NO_MOVE = _lib.BLOB_NO_MOVE


def check_args(W, H, n, connectivity=8, min_area=1, max_blobs=4096):
    """the library's own decision on the arguments (ofc_blob_check, host only): ValueError or OfcError as it refuses"""
    check(load().ofc_blob_check(int(W), int(H), int(n), int(connectivity), int(min_area), int(max_blobs)))


def order_records(slots, found, max_blobs):
    """a pair's records as the device left them (its first min(found, max_blobs) slots, in no order) -> the table of the
    definition: (n,12) int64 ascending by root; no record at all when found > max_blobs"""
    slots = np.asarray(slots, np.int64).reshape(-1, NF)
    if found > max_blobs:
        return np.zeros((0, NF), np.int64)
    rec = slots[:found]
    return np.ascontiguousarray(rec[np.argsort(rec[:, 0], kind="stable")])


def select_mask(select, k):
    """None (every label) or an iterable of labels < k -> the bit mask ofc_blob_keys_dev takes"""
    if select is None:
        return (1 << k) - 1
    mask = 0
    for lab in select:
        if not 0 <= int(lab) < k:
            raise ValueError(f"select names label {lab}, the model has {k}")
        mask |= 1 << int(lab)
    return mask


class Blobs:
    """labels: (n,H,W) int32 (root per foreground pixel, -1 background) or None; records: per pair an (n_i,12) int64 array,
    columns FIELDS, ascending by root; found: (n,) int32, the components with area >= min_area (records[i] is empty when
    found[i] > max_blobs); keys: the (n,H,W) u8 key map when it was built from a field, else None.
    With links (link, components_dev(links=), FlowStream): links is a list of n-1 (m_t,3) int64 arrays, columns LINK_FIELDS,
    ascending by (root_a, root_b), transition t leading from pair t to pair t+1; nlinks (n-1,) int32 is m_t, or -1 where the
    transition had more than max_links distinct links and delivers none; moves the (n,H,W) int32 move words where they were
    built from a host field.  Without links all three are None."""

    def __init__(self, W, H, labels, records, found, keys=None):
        self.W, self.H, self.labels, self.records, self.found, self.keys = W, H, labels, records, found, keys
        self.links = self.nlinks = self.moves = None

    def __len__(self):
        return len(self.records)

    def boxes(self, i):
        """(n_i,4) int64: xmin, ymin, xmax, ymax, inclusive"""
        return self.records[i][:, 3:7]

    def centroids(self, i):
        """(n_i,2) f64: Sx / area, Sy / area"""
        r = self.records[i]
        return r[:, 7:9] / r[:, 2:3].astype(np.float64)

    def mean_flow(self, i):
        """(n_i,2) f64: the mean of the component's valid vectors, Sq / nvalid / 65536; NaN where it has none"""
        r = self.records[i]
        with np.errstate(invalid="ignore", divide="ignore"):
            return r[:, 10:12] / r[:, 9:10].astype(np.float64) / 65536.0

    def rows(self, tracks=None):
        """one row per blob in CSV_HEADER's order: what motionGrids --blobs writes.  With a Tracks (tracks(self)) the blob's
        track id is appended as a last column: TRACK_CSV_HEADER's order, what --tracks writes."""
        out = []
        for i, r in enumerate(self.records):
            cen, mf = self.centroids(i), self.mean_flow(i)
            for j, b in enumerate(r.tolist()):
                row = (i, b[1], b[0] % self.W, b[0] // self.W, b[2], b[3], b[4], b[5], b[6],
                       "%.3f" % cen[j, 0], "%.3f" % cen[j, 1], "%.4f" % mf[j, 0], "%.4f" % mf[j, 1])
                out.append(row if tracks is None else row + (int(tracks.ids[i][j]),))
        return out


def _stack_keys(keys):
    k = np.ascontiguousarray(keys, np.uint8)
    if k.ndim == 2:
        k = k[None]
    if k.ndim != 3 or k.size == 0:
        raise ValueError(f"keys should be (H,W) or (n,H,W) uint8, got shape {k.shape}")
    return k


def _stack_flow(flow):
    f = np.ascontiguousarray(flow, np.float32)
    if f.ndim == 3:
        f = f[None]
    if f.ndim != 4 or f.shape[3] != 2 or f.size == 0:
        raise ValueError(f"flow should be (H,W,2) or (n,H,W,2), got shape {f.shape}")
    return f


def _run(keys, flow, keyargs, connectivity, min_area, max_blobs, labels, device):
    n, H, W = (keys if keys is not None else flow).shape[:3]
    check_args(W, H, n, connectivity, min_area, max_blobs)
    use_thr, thr, k, mean, cen_c, select, merge = keyargs
    lab = np.empty((n, H, W), np.int32) if labels else None
    kout = np.empty((n, H, W), np.uint8) if keys is None else None
    table = np.empty((n, max_blobs, NF), np.int64)
    cnt, found = np.empty(n, np.int32), np.empty(n, np.int32)
    check(load().ofc_blobs(device, ptr(keys), ptr(flow), W, H, n, use_thr, thr, k, ptr(mean), ptr(cen_c), select, merge,
                           connectivity, min_area, max_blobs, ptr(lab), ptr(kout), ptr(table), ptr(cnt), ptr(found)))
    recs = [order_records(table[i, :cnt[i]], int(cnt[i]), max_blobs) for i in range(n)]
    return Blobs(W, H, lab, recs, found, kout)


NO_KEYS = (0, 0.0, 0, None, None, 0, 0)


def connected_components(keys, connectivity=8, min_area=1, max_blobs=4096, flow=None, labels=True, device=0):
    """keys (H,W) or (n,H,W) u8, 255 = background -> Blobs.  flow ((n,)H,W,2 f32) feeds the records' nvalid, squ, sqv
    (Blobs.mean_flow); without it they are 0.  labels=False skips the label map's copy to the host."""
    k = _stack_keys(keys)
    f = None if flow is None else _stack_flow(flow)
    if f is not None and f.shape[:3] != k.shape:
        raise ValueError(f"flow {f.shape} does not match keys {k.shape}")
    return _run(k, f, NO_KEYS, connectivity, min_area, max_blobs, labels, device)


def moving_blobs(flow, thr=0.5, connectivity=8, min_area=1, max_blobs=4096, labels=True, device=0):
    """the regions of a field that move: foreground where u*u + v*v >= thr*thr in f32 (the ('moving', thr) weight's test),
    all with key 0 -> Blobs.  On hand-held footage run camera.compensate first."""
    return _run(None, _stack_flow(flow), (1, float(thr), 0, None, None, 0, 0), connectivity, min_area, max_blobs, labels, device)


def cluster_blobs(flow, centers, select=None, merge=False, mean=None, thr=None, connectivity=8, min_area=1, max_blobs=4096,
                  labels=True, device=0):
    """the regions of a field by motion cluster: every vector gets the label L the E-step gives it against `centers`
    ((k,2), un-centred; the arithmetic centred by `mean`, None = (0, 0), as vis.grid_assign_counts), is foreground iff L
    is in `select` (None: every label) and, with thr, iff it also moves; key = L, so neighbouring regions of different
    motion stay apart, or 0 with merge=True, which joins them -> Blobs"""
    from .vis import _model_args
    k, mean, cen_c = _model_args(centers, mean)
    mask = select_mask(select, min(k, 16))                # the library refuses k > 16
    args = (int(thr is not None), float(thr or 0.0), k, mean, cen_c, mask, int(bool(merge)))
    return _run(None, _stack_flow(flow), args, connectivity, min_area, max_blobs, labels, device)


def components_dev(keys_ptr, flow_ptr, W, H, n, connectivity=8, min_area=1, max_blobs=4096, labels=True, device=0, links=None,
                   moves_ptr=None):
    """connected_components on a key map and (optionally, 0 / None) a field that are already on the device: u8 [n][H][W]
    at keys_ptr, f32 [n][H][W][2] at flow_ptr.  Only the label map (if asked for) and the records leave it.
    links = a max_links: the blobs are linked across the n - 1 transitions as well (Blobs.links, Blobs.nlinks), by the
    moves int32 [n][H][W] at moves_ptr (moves_dev), or, without moves_ptr, by moves taken from the field at flow_ptr as it
    stands, which must then be the field that says where pixels go, not a residual."""
    check_args(W, H, n, connectivity, min_area, max_blobs)
    if links is not None:
        check_link_args(W, H, n, min_area, links)
        if not moves_ptr and not flow_ptr:
            raise ValueError("links need moves_ptr or a field at flow_ptr")
    P = W * H
    lab = DeviceBuffer(n * P * 4, device)
    tab = DeviceBuffer(n * max_blobs * NF * 8, device)
    fnd = DeviceBuffer(n * 4, device)
    try:
        L = load()
        check(L.ofc_blob_label_dev(device, C.c_void_p(keys_ptr), W, H, n, connectivity, C.c_void_p(lab.ptr)))
        check(L.ofc_blob_table_dev(device, C.c_void_p(keys_ptr), C.c_void_p(lab.ptr), C.c_void_p(flow_ptr) if flow_ptr else None,
                                   W, H, n, min_area, max_blobs, C.c_void_p(tab.ptr), C.c_void_p(fnd.ptr)))
        found = fnd.download((n,), np.int32)
        recs = []
        for i in range(n):
            have = int(found[i]) if found[i] <= max_blobs else 0
            raw = tab.download((have, NF), np.int64, offset=i * max_blobs * NF * 8) if have else np.zeros((0, NF), np.int64)
            recs.append(order_records(raw, int(found[i]), max_blobs))
        out = Blobs(W, H, lab.download((n, H, W), np.int32) if labels else None, recs, found)
        if links is not None:
            own = None
            try:
                if not moves_ptr:
                    own = DeviceBuffer(n * P * 4, device)
                    moves_dev(flow_ptr, W, H, n, own.ptr, device)
                out.links, out.nlinks = links_dev(lab.ptr, moves_ptr or own.ptr, W, H, n, min_area, links, device)
            finally:
                if own is not None:
                    own.free()
        return out
    finally:
        for b in (lab, tab, fnd):
            b.free()


def keys_dev(flow_ptr, W, H, n, keys_ptr, thr=None, centers=None, mean=None, select=None, merge=False, device=0):
    """ofc_blob_keys_dev on a resident field: the key map of moving_blobs (centers None) or cluster_blobs into keys_ptr"""
    k, cen_c, mask = 0, None, 0
    if centers is not None:
        from .vis import _model_args
        k, mean, cen_c = _model_args(centers, mean)
        mask = select_mask(select, min(k, 16))
    check(load().ofc_blob_keys_dev(device, C.c_void_p(flow_ptr), W, H, n, int(thr is not None), float(thr or 0.0), k,
                                   ptr(mean) if k else None, ptr(cen_c), mask, int(bool(merge)), C.c_void_p(keys_ptr)))


# ---- links between the blobs of consecutive pairs, and the tracks they give (csrc/blob_links.hip) ----
def check_link_args(W, H, n, min_area=1, max_links=4096):
    """the library's own decision on the link arguments (ofc_blob_link_check, host only): ValueError or OfcError"""
    check(load().ofc_blob_link_check(int(W), int(H), int(n), int(min_area), int(max_links)))


def _split_links(table, nlinks):
    """ofc_blob_links_read's output -> the list Blobs.links holds"""
    return [np.ascontiguousarray(table[t, :max(int(m), 0)]) for t, m in enumerate(nlinks)]


def moves_dev(flow_ptr, W, H, n, moves_ptr, device=0):
    """ofc_blob_moves_dev on a resident field f32 [n][H][W][2]: its move words, int32 [n][H][W], into moves_ptr.  Take them
    from the field that says where pixels go: before the camera is subtracted from it."""
    check(load().ofc_blob_moves_dev(device, C.c_void_p(flow_ptr), W, H, n, C.c_void_p(moves_ptr)))


def links_dev(labels_ptr, moves_ptr, W, H, n, min_area=1, max_links=4096, device=0):
    """the links of label maps int32 [n][H][W] at labels_ptr (ofc_blob_label_dev's) under the moves int32 [n][H][W] at
    moves_ptr, both on the device -> (links: n-1 arrays (m_t,3) int64, nlinks (n-1,) int32).  Only the tables leave it."""
    check_link_args(W, H, n, min_area, max_links)
    ntrans = n - 1
    table, nlinks = np.zeros((ntrans, max_links, LINK_NF), np.int64), np.zeros(ntrans, np.int32)
    if ntrans == 0:
        return [], nlinks
    L = load()
    tab = DeviceBuffer(L.ofc_blob_links_bytes(max_links, ntrans), device)
    cnt = DeviceBuffer(max(ntrans * 4, 8), device)
    try:
        check(L.ofc_blob_links_dev(device, C.c_void_p(labels_ptr), C.c_void_p(moves_ptr), W, H, n, min_area, max_links,
                                   C.c_void_p(tab.ptr), C.c_void_p(cnt.ptr)))
        check(L.ofc_blob_links_read(device, C.c_void_p(tab.ptr), C.c_void_p(cnt.ptr), ntrans, max_links, ptr(table), ptr(nlinks)))
    finally:
        tab.free()
        cnt.free()
    return _split_links(table, nlinks), nlinks


def link(b, flow, min_area=1, max_links=4096, device=0):
    """fills the links of a Blobs that has its label map (b.links, b.nlinks, b.moves) and returns it.  A pixel of blob a in
    pair t lands, by its own flow vector rounded to whole pixels, on a pixel of pair t+1; the label there is a vote for "a
    continues as b".  `flow` ((n,)H,W,2 f32) is the field that says where pixels go: the flow BEFORE camera.compensate, not
    the residual the blobs may have been keyed on.  min_area should be the one the Blobs was made with: only blobs of at
    least that area vote or are voted for.  A transition with more than max_links distinct links delivers none
    (nlinks = -1)."""
    if b.labels is None:
        raise ValueError("link needs the label map: make the Blobs with labels=True")
    f = _stack_flow(flow)
    lab = np.ascontiguousarray(b.labels, np.int32)
    if f.shape[:3] != lab.shape:
        raise ValueError(f"flow {f.shape} does not match the label map {lab.shape}")
    n, H, W = lab.shape
    check_link_args(W, H, n, min_area, max_links)
    moves = np.empty((n, H, W), np.int32)
    table, nlinks = np.zeros((n - 1, max_links, LINK_NF), np.int64), np.zeros(n - 1, np.int32)
    check(load().ofc_blob_links(device, ptr(lab), ptr(f), W, H, n, min_area, max_links, ptr(moves), ptr(table), ptr(nlinks)))
    b.links, b.nlinks, b.moves = _split_links(table, nlinks), nlinks, moves
    return b


class Tracks:
    """ids: per pair an int64 array parallel to the Blobs' records[i], the track each blob belongs to; n_tracks: how many
    ids were handed out; broken: the transitions that broke every track through them"""

    def __init__(self, ids, n_tracks, broken):
        self.ids, self.n_tracks, self.broken = ids, n_tracks, broken

    def lengths(self):
        """(n_tracks,) int64: in how many pairs each track appears"""
        out = np.zeros(self.n_tracks, np.int64)
        for i in self.ids:
            np.add.at(out, i, 1)
        return out


def _best(links, own, other):
    """per distinct links[:, own] the row with the most votes, ties to the smaller links[:, other] -> {root: root}"""
    out = {}
    for j in np.lexsort((links[:, other], -links[:, 2], links[:, own])):
        out.setdefault(int(links[j, own]), int(links[j, other]))
    return out


def tracks(b, min_votes=1):
    """track ids over a Blobs that carries links -> Tracks.  Within a transition only links with votes >= min_votes whose two
    roots both have a record count; succ(a) is a's link with the most votes (ties: the smaller root_b), pred(b) is b's
    (ties: the smaller root_a), and (a, b) is accepted iff succ(a) = b and pred(b) = a.  Ids are int64, handed out in
    (pair, root) order: pair 0's blobs get 0, 1, ...; a later blob with an accepted predecessor takes the predecessor's id,
    every other blob the next unused integer.  A transition breaks every track through it when it overflowed
    (nlinks = -1) or when either of its pairs overflowed its blob table (found > max_blobs: it has no records): all blobs of
    the later pair start new ids.
    Splits and merges are not modelled: where a blob splits, or two merge, the larger share keeps the id and the other
    part starts a new one (or ends)."""
    if b.links is None:
        raise ValueError("the Blobs carries no links: blobs.link, components_dev(links=) or a stream with max_links")
    ids, broken, nxt = [], [], 0
    for i, rec in enumerate(b.records):
        roots = rec[:, 0]
        cur = np.full(len(roots), -1, np.int64)
        if i > 0:
            t = i - 1
            over = [int(b.found[j]) != len(b.records[j]) for j in (t, i)]
            if b.nlinks[t] < 0 or any(over):
                broken.append(t)
            else:
                lk = b.links[t]
                lk = lk[(lk[:, 2] >= min_votes) & np.isin(lk[:, 0], b.records[t][:, 0]) & np.isin(lk[:, 1], roots)]
                succ, pred = _best(lk, 0, 1), _best(lk, 1, 0)
                before = {int(r): int(k) for r, k in zip(b.records[t][:, 0], ids[t])}
                for j, r in enumerate(roots.tolist()):
                    a = pred.get(r)
                    if a is not None and succ[a] == r:
                        cur[j] = before[a]
        for j in range(len(cur)):
            if cur[j] < 0:
                cur[j] = nxt
                nxt += 1
        ids.append(cur)
    return Tracks(ids, nxt, broken)
