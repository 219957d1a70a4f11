"""Host side of the super-quadric multi-view fit: thin Python over the C ABI (include/odam_sq.h).

Mirrors the pieces of the reference (likojack/ODAM) that sit around SuperQuadricOptimizer.run:
  src/super_quadric/sq_libs.py:353-393  (init: scales -> sqrt(dims/2), shapes = -0 / -10000, prior table)
  src/super_quadric/sq_libs.py:438-451  (gt / mask arrays per direction)
  src/super_quadric/sq_libs.py:13-22    (CLASS_MAPPER order of the prior rows)
"""
import ctypes
import os
import pickle
import threading

import numpy as np
import torch

from . import _lib

N_POINTS = 1000
WG_VIEWS = 1024          # rows one workgroup reduces (ODAM_SQ_MAX_VIEWS)
MAX_VIEWS = 16 * WG_VIEWS  # per object: split over up to 16 workgroups
NAMES = ("x_min", "x_max", "y_min", "y_max")  # sq_libs.py:438
REPRESENTATIONS = {"super_quadric": 0, "cube": 1, "quadric": 2, "dual_quadric": 3}   # 0..2: odam_sq_fit_batch codes; 3: fit_dual
STATE_FLOATS = 32        # ODAM_SQ_STATE_FLOATS: parameters 0..8, exp_avg 9..17, exp_avg_sq 18..26, scales_init 27..29, steps 30, representation 31
DQ_POINTS = 2500         # 50 x 50 angle grid of DualQuadric.compute_ellipsoid_points (sq_libs.py:325)
# sq_libs.py:13-22
CLASS_MAPPER = {0: "03211117", 1: "04379243", 2: "02808440", 3: "02747177",
                4: "04256520", 5: "03001627", 6: "02933112", 7: "02871439"}

_PRIOR_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "scale_prior.npz")


def load_scale_prior(path=None):
    """[8, 9] float32 inverse covariances in CLASS_MAPPER order.

    `path` may be the reference's pickle (src/super_quadric/scale_prior, a dict synset -> 3x3
    float64) or None for the copy of those 72 numbers shipped in odam_amd/data/scale_prior.npz.
    """
    if path is None:
        z = np.load(_PRIOR_PATH)
        return z["icov"].astype(np.float32).reshape(8, 9)
    with open(path, "rb") as f:
        d = pickle.load(f)
    return np.stack([np.asarray(d[CLASS_MAPPER[k]], np.float64).astype(np.float32).reshape(9)
                     for k in range(8)])


def lines_to_targets(bbox_lines):
    """list (per valid frame) of {name: [a, b, -pixel]} -> tgt[F,4], mask[F,4] float32 (sq_libs.py:438-451)."""
    F = len(bbox_lines)
    tgt = np.zeros((F, 4), np.float32)
    mask = np.zeros((F, 4), np.float32)
    for f, d in enumerate(bbox_lines):
        for k, name in enumerate(NAMES):
            if name in d:
                mask[f, k] = 1.0
                # gt = float32(line[-1]) = -pixel; the residual compares with -gt
                tgt[f, k] = -np.float32(d[name][-1])
    return tgt, mask


def init_params(translate, angle, dims, representation="super_quadric"):
    """SuperQuadricOptimizer.__init__ (sq_libs.py:353-371): 9 float32 parameters."""
    scales = np.sqrt(np.asarray(dims, np.float64) / 2)
    shapes = np.array([-10000.0, -10000.0]) if representation == "cube" else np.array([-0.0, -0.0])
    return np.concatenate([np.asarray(translate, np.float64).reshape(3), [float(angle)], scales,
                           shapes]).astype(np.float32)


# odam_sq_fit_resume as include/odam_sq.h declares it (tests/test_sq_resume_host.py holds the two together)
FIT_RESUME_ARGTYPES = ([ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 7 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 8)


def _fit_resume_entry():
    f = _lib.lib().odam_sq_fit_resume
    if f.argtypes is None:
        f.argtypes, f.restype = FIT_RESUME_ARGTYPES, ctypes.c_int
    return f


# odam_dq_svd_batch as include/odam_sq.h declares it (tests/test_quadric_svd_host.py holds the two together)
DQ_SVD_ARGTYPES = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 4


def _dq_svd_entry():
    f = _lib.lib().odam_dq_svd_batch
    if f.argtypes is None:
        f.argtypes, f.restype = DQ_SVD_ARGTYPES, ctypes.c_int
    return f


# the reprojection entry points as include/odam_sq.h declares them (tests/test_reproject_host.py holds the two together)
_VP, _CI = ctypes.c_void_p, ctypes.c_int
REPROJECT_ARGTYPES = {
    "odam_sq_reproject_batch": [_VP, _CI, _VP, _CI, _VP, _VP, _CI, _VP, _VP, _VP],
    "odam_dq_reproject_batch": [_VP, _CI, _VP, _VP, _VP, _CI, _VP, _VP, _VP],
    "odam_reproject_score_f32": [_VP, _CI] + [_VP] * 5 + [ctypes.c_float] * 2 + [_CI] + [_VP] * 5,
    "odam_reproject_score_f64": [_VP, _CI] + [_VP] * 5 + [ctypes.c_double] * 2 + [_CI] + [_VP] * 5,
}


def _reproject_entry(name):
    f = getattr(_lib.lib(), name)
    if f.argtypes is None:
        f.argtypes, f.restype = REPROJECT_ARGTYPES[name], ctypes.c_int
    return f


# odam_sq_prepare_batch as include/odam_sq.h declares it (tests/test_sq_prepare_host.py holds the two together)
_CD = ctypes.c_double
PREPARE_ARGTYPES = [_VP, _CI, _VP, _VP, _CI, _CI, _VP, _VP, _VP, _CD, _CD, _CD, _CI] + [_VP] * 15
PREPARE_MAX_ROWS = 16384      # ODAM_SQ_PREPARE_MAX_ROWS: rows of one track the prelude kernel sorts
PREPARE_NO_VIEW, PREPARE_BAD_CLASS, PREPARE_TOO_MANY_ROWS = 1, 2, 3      # its status codes
EDGE_THRESHOLD = 20           # tracking_gt_utils.py:199


def _prepare_entry():
    f = _lib.lib().odam_sq_prepare_batch
    if f.argtypes is None:
        f.argtypes, f.restype = PREPARE_ARGTYPES, ctypes.c_int
    return f


# odam_sq_prepare_scenes as include/odam_sq.h declares it (tests/test_map_scenes_host.py holds the two together)
PREPARE_SCENES_ARGTYPES = [_VP, _CI, _VP, _VP, _CI, _CI, _VP, _VP, _CI, _VP, _VP, _VP, _VP, _VP, _CD, _CI] + [_VP] * 15


def _prepare_scenes_entry():
    f = _lib.lib().odam_sq_prepare_scenes
    if f.argtypes is None:
        f.argtypes, f.restype = PREPARE_SCENES_ARGTYPES, ctypes.c_int
    return f


# odam_merge_cluster / odam_merge_assemble as include/odam_merge.h declares them (tests/test_track_merge_host.py holds them together)
_LL = ctypes.c_longlong
MERGE_ARGTYPES = {
    "odam_merge_cluster": [_VP, _CI, _VP, _VP, _CI, _LL, _CI, _VP, _CD, _VP, _VP, _VP, _VP, _VP, _VP],
    "odam_merge_assemble": [_VP, _CI, _VP, _CI, _VP, _VP, _VP, _VP, _VP, _CI, _CI, _VP, _VP, _VP, _CI] + [_VP] * 9,
}
MERGE_MAX_TRACKS = 1024       # ODAM_MERGE_MAX_TRACKS: tracks of one scene the clustering kernel takes
MERGE_THRESHOLD = 0.95        # run_merge.py:121


def _merge_entry(name):
    f = getattr(_lib.lib(), name)
    if f.argtypes is None:
        f.argtypes, f.restype = MERGE_ARGTYPES[name], ctypes.c_int
    return f


def unique_frame_ids(img_names):
    """img_names as int64 where every frame id names ONE image -- at least one id, all different, inside int32 -- else None: the rule
    under which multi_view._UniqueFrames and odam_sq_prepare_batch find a row's image by binary search"""
    names = np.asarray([int(f) for f in img_names], np.int64)
    if not len(names) or len(np.unique(names)) != len(names) or np.abs(names).max() >= 2 ** 31:
        return None
    return names


def frame_tables(img_names):
    """img_names -> (ids int64 ascending, order int32: image index of ids[i]), the two tables odam_sq_prepare_batch searches (and
    multi_view._UniqueFrames holds); ValueError unless unique_frame_ids accepts the names"""
    names = unique_frame_ids(img_names)
    if names is None:
        raise ValueError("prepare: the frame ids of img_names must be all different, inside int32, and at least one")
    order = np.argsort(names, kind="stable")
    return names[order], order.astype(np.int32)


def cold_state(params0, representation):
    """[n, 32] float32 rows of fits that have not begun (include/odam_sq.h): what a track that starts cold gets inside a resumed call"""
    p = np.asarray(params0, np.float32).reshape(-1, 9)
    st = np.zeros((len(p), STATE_FLOATS), np.float32)
    st[:, 0:9] = p
    st[:, 27:30] = p[:, 4:7]
    st[:, 31] = REPRESENTATIONS[representation]
    return st


class SqFitter:
    """Owns the device context (constant sampler draws + Adam tables)."""

    def __init__(self, device="cuda:0", max_iters=200):
        self.device = torch.device(device)
        self.max_iters = int(max_iters)
        L = _lib.lib()
        with torch.cuda.device(self.device):
            h = ctypes.c_void_p()
            _lib.check(L.odam_sq_create(ctypes.c_int(self.max_iters), ctypes.byref(h)), "odam_sq_create")
        self._h = h
        self._prior = None
        # The native handle serves ONE launch at a time (include/odam_sq.h): its view-split exchange buffer is per
        # handle.  The lock serialises host threads; launches from different streams are additionally ordered by an
        # event so that a second fit cannot start writing exchange slots while the first still polls them.
        self._lock = threading.Lock()
        self._last = None          # (stream id, event) of the most recent launch
        with torch.cuda.device(self.device):
            self.n_cu = int(torch.cuda.get_device_properties(self.device).multi_processor_count)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().odam_sq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _prior_dev(self):
        if self._prior is None:
            self._prior = torch.from_numpy(load_scale_prior()).to(self.device).contiguous()
        return self._prior

    def fit(self, params0, class_ids, view_counts, P, tgt, mask, n_iters=200, representation="super_quadric",
            prior=True, want_points=True, want_loss=False, want_traj=False, state=None, want_state=False):
        """Batched SuperQuadricOptimizer.run.

        params0 [n,9] f32; class_ids [n] int; view_counts [n] int; P [sumF,3,4]/[sumF,12] f32;
        tgt, mask [sumF,4] f32 (numpy or torch, host or device).  Returns dict of device tensors.

        Objects with more than 1024 views need the library's view split (k workgroups per object, k x padded object
        count <= number of CUs): they are fitted in groups small enough for that; fits are independent, so the
        grouping does not change any result.

        Resumable fits (odam_sq_fit_resume): with want_state the dict also holds "state", a device tensor [n, 32] (layout in
        include/odam_sq.h); passed back as `state` (host or device, numpy or torch) the fit continues where that one stopped --
        params0 is then ignored, the views may have changed, loss / traj hold the new steps only -- and k steps followed by n - k
        resumed steps on the same views are the bits of n steps.  The steps taken so far and the representation are read from the
        state (a small copy to the host for a device tensor); more than max_iters steps in all, or a state of another
        representation, is refused before anything is launched.  Without either argument this is the call it always was.
        """
        vc = np.asarray(view_counts, np.int64)
        resumable = state is not None or want_state
        st = t0 = None
        if state is not None:
            st, t0 = self._check_state(state, len(vc), int(n_iters), representation)
        if len(vc) and vc.max() > WG_VIEWS:
            return self._fit_grouped(params0, class_ids, vc, P, tgt, mask, dict(
                n_iters=n_iters, representation=representation, prior=prior, want_points=want_points,
                want_loss=want_loss, want_traj=want_traj), state=st, t0=t0, want_state=want_state)
        if resumable:
            return self._fit_once(params0, class_ids, view_counts, P, tgt, mask, n_iters, representation, prior,
                                  want_points, want_loss, want_traj, state=st, t0=t0, want_state=want_state)
        return self._fit_once(params0, class_ids, view_counts, P, tgt, mask, n_iters, representation, prior,
                              want_points, want_loss, want_traj)

    def _check_state(self, state, n, n_iters, representation):
        """-> (device tensor [n, 32], host int32 array of the steps taken): the refusals that need the state's own words"""
        if representation not in REPRESENTATIONS or REPRESENTATIONS[representation] > 2:
            raise ValueError(f"a fit of representation {representation!r} cannot be resumed (super_quadric, cube and quadric can)")
        st = state if torch.is_tensor(state) else torch.as_tensor(np.ascontiguousarray(state, np.float32))
        if st.dim() != 2 or tuple(st.shape) != (n, STATE_FLOATS):
            raise ValueError(f"state must be [{n}, {STATE_FLOATS}] (one row per object), got {tuple(st.shape)}")
        st = st.to(device=self.device, dtype=torch.float32).contiguous()
        tail = st[:, 30:32].cpu().numpy()
        rep = REPRESENTATIONS[representation]
        bad = np.flatnonzero(tail[:, 1] != rep)
        if len(bad):
            names = {v: k for k, v in REPRESENTATIONS.items()}
            was = names.get(int(tail[bad[0], 1]), repr(float(tail[bad[0], 1])))
            raise ValueError(f"state row {int(bad[0])} belongs to a fit of representation {was!r}, this call fits {representation!r}")
        t0 = tail[:, 0].astype(np.int32)
        if n and ((tail[:, 0] != t0) | (t0 < 0)).any():
            raise ValueError("state word 30 (steps taken) is not a non-negative integer")
        if n and int(t0.max()) + n_iters > self.max_iters:
            i = int(t0.argmax())
            raise _lib.OdamError(f"resumed fit: object {i} has taken {int(t0[i])} steps, {n_iters} more make {int(t0[i]) + n_iters} > "
                                 f"max_iters {self.max_iters} of this SqFitter (code 3)")
        return st, t0

    def _fit_grouped(self, params0, class_ids, vc, P, tgt, mask, kw, state=None, t0=None, want_state=False):
        if vc.max() > MAX_VIEWS:
            raise _lib.OdamError(f"views per object must be in 1..{MAX_VIEWS}, got {vc.min()}..{vc.max()}")
        as_t = lambda x: x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        P, tgt, mask, params0 = as_t(P).reshape(-1, 12), as_t(tgt).reshape(-1, 4), as_t(mask).reshape(-1, 4), as_t(params0).reshape(-1, 9)
        offs = np.concatenate([[0], np.cumsum(vc)])
        need = np.ones(len(vc), np.int64)                      # workgroups an object needs
        big = vc > WG_VIEWS
        need[big] = (2 ** np.ceil(np.log2(vc[big])).astype(np.int64)) // WG_VIEWS
        groups = [np.flatnonzero(~big)] if (~big).any() else []
        for k in sorted(set(need[big].tolist())):
            idx = np.flatnonzero(need == k)
            per = max(8, (self.n_cu // k) // 8 * 8)            # padded object count x k <= number of CUs
            groups += [idx[i:i + per] for i in range(0, len(idx), per)]
        outs = {}
        for g in groups:
            rows = np.concatenate([np.arange(offs[i], offs[i + 1]) for i in g])
            more = {}
            if state is not None or want_state:      # the state travels like every other per-object tensor: gathered here, scattered below
                more = dict(state=None if state is None else state[torch.as_tensor(g, device=state.device)],
                            t0=None if t0 is None else t0[g], want_state=want_state)
            o = self._fit_once(params0[g], [class_ids[i] for i in g], vc[g], P[rows], tgt[rows], mask[rows],
                               kw["n_iters"], kw["representation"], kw["prior"], kw["want_points"], kw["want_loss"], kw["want_traj"], **more)
            for key, val in o.items():
                if val is None:
                    outs[key] = None
                    continue
                if key not in outs:
                    outs[key] = torch.empty((len(vc),) + tuple(val.shape[1:]), device=val.device, dtype=val.dtype)
                outs[key][torch.as_tensor(g, device=val.device)] = val
        return outs

    def _fit_once(self, params0, class_ids, view_counts, P, tgt, mask, n_iters=200, representation="super_quadric",
                  prior=True, want_points=True, want_loss=False, want_traj=False, state=None, t0=None, want_state=False):
        dev = self.device
        n = len(view_counts)
        resumable = state is not None or want_state
        as_dev = lambda x, dt: torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(
            device=dev, dtype=dt).contiguous()
        vc = np.asarray(view_counts, np.int64)
        if n == 0:
            out = {"params": torch.zeros(0, 9, device=dev), "points": torch.zeros(0, N_POINTS, 3, device=dev)}
            if want_state:
                out["state"] = torch.zeros(0, STATE_FLOATS, device=dev)
            return out
        if vc.min() < 1 or vc.max() > MAX_VIEWS:
            raise _lib.OdamError(f"views per object must be in 1..{MAX_VIEWS}, got {vc.min()}..{vc.max()}")
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum(vc)
        d_p0 = as_dev(params0, torch.float32).reshape(n, 9) if (state is None or params0 is not None) else None
        cls = np.asarray(class_ids, np.int32).copy()
        if prior:
            if cls.min() < 0 or cls.max() > 7:
                raise KeyError(int(cls.max()))  # CLASS_MAPPER covers 0..7 only (sq_libs.py:464)
        else:
            cls[:] = -1
        d_cls = as_dev(cls, torch.int32)
        d_off = as_dev(offs, torch.int32)
        d_P = as_dev(P, torch.float32).reshape(-1, 12)
        d_t = as_dev(tgt, torch.float32).reshape(-1, 4)
        d_m = as_dev(mask, torch.float32).reshape(-1, 4)
        assert d_P.shape[0] == offs[-1] and d_t.shape[0] == offs[-1] and d_m.shape[0] == offs[-1]
        out_p = torch.empty(n, 9, device=dev, dtype=torch.float32)
        out_pts = torch.empty(n, N_POINTS, 3, device=dev, dtype=torch.float32) if want_points else None
        loss = torch.empty(n, n_iters, device=dev, dtype=torch.float32) if want_loss else None
        traj = torch.empty(n, n_iters, 9, device=dev, dtype=torch.float32) if want_traj else None
        st_out = torch.empty(n, STATE_FLOATS, device=dev, dtype=torch.float32) if want_state else None
        h_t0 = None if state is None else np.ascontiguousarray(t0, np.int32)
        with torch.cuda.device(dev), self._lock:
            cur = torch.cuda.current_stream(dev)
            stream = cur.cuda_stream
            if self._last is not None and self._last[0] != stream:
                cur.wait_event(self._last[1])     # the handle's previous launch ran on another stream: order behind it
            if resumable:
                _lib.check(_fit_resume_entry()(
                    self._h, int(n), _lib.ptr(d_p0), _lib.ptr(d_cls), _lib.ptr(d_off), _lib.ptr(d_P),
                    _lib.ptr(d_t), _lib.ptr(d_m), _lib.ptr(self._prior_dev()), int(n_iters),
                    REPRESENTATIONS[representation], int(vc.max()),
                    _lib.ptr(out_p), _lib.ptr(out_pts), _lib.ptr(loss), _lib.ptr(traj),
                    _lib.ptr(state), None if h_t0 is None else h_t0.ctypes.data_as(ctypes.c_void_p), _lib.ptr(st_out),
                    ctypes.c_void_p(stream)), "odam_sq_fit_resume")
            else:
                _lib.check(_lib.lib().odam_sq_fit_batch(
                    self._h, ctypes.c_int(n), _lib.ptr(d_p0), _lib.ptr(d_cls), _lib.ptr(d_off), _lib.ptr(d_P),
                    _lib.ptr(d_t), _lib.ptr(d_m), _lib.ptr(self._prior_dev()), ctypes.c_int(int(n_iters)),
                    ctypes.c_int(REPRESENTATIONS[representation]), ctypes.c_int(int(vc.max())),
                    _lib.ptr(out_p), _lib.ptr(out_pts), _lib.ptr(loss), _lib.ptr(traj),
                    ctypes.c_void_p(stream)), "odam_sq_fit_batch")
            ev = torch.cuda.Event()
            ev.record(cur)
            self._last = (stream, ev)
        out = {"params": out_p, "points": out_pts, "loss": loss, "traj": traj}
        if want_state:
            out["state"] = st_out
        return out

    def prepare(self, rows, row_offsets, img_names, P_cws, img_h, img_w, representation="super_quadric", thr=EDGE_THRESHOLD, max_rows=None):
        """The prelude of a fit pass for ALL tracks in one launch (include/odam_sq.h, odam_sq_prepare_batch): views, constraint rows,
        class, detector box and initial parameters of every track.

        rows [R, 14] float64: the first 14 columns of every track row, track after track; row_offsets [n + 1]: track o owns rows
        row_offsets[o] .. row_offsets[o + 1] - 1 (numpy or torch, on the host or the device; offsets given on the host are checked
        and size the launch, offsets on the device are taken as they are and the launch is sized for the largest track the kernel
        takes, or for max_rows, the most rows of one track, where the caller knows it (track_store.TrackRows does) -- nothing is read
        back for them; a track with more rows than the launch is sized for gets status 3); img_names: the frame id of every image, all different; P_cws [n_img, 3, 4].
        Returns a dict: "cls", "n_obs", "n_valid", "status" [n] int32 numpy on the host -- ONE small copy, the only synchronisation
        -- and device tensors "init" ([n, 9], or [n, 5] with "half_dims" [n, 3] for "dual_quadric"; else half_dims is None), "pose"
        [n, 7] and "bboxes_dl" [n, 8, 3] float64, per view from row_offsets[o] on "view_img", "view_row", "valid" [R] int32, "tgt",
        "mask" [R, 4], "P" [R, 12] float32, and "row_offsets" [n + 1] int32.  Rows of a per-track output whose status says it was
        not written, and per-view words beyond a track's n_obs views (fewer than its rows where a frame id repeats or names no image),
        are uninitialised memory -- except "valid", which is 0 there: (valid != 0) marks the constrained views among all R rows."""
        dev = self.device
        rep = REPRESENTATIONS[representation]
        ids, order = frame_tables(img_names)
        if torch.is_tensor(row_offsets) and row_offsets.is_cuda:
            d_off = row_offsets.to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
            max_rows = PREPARE_MAX_ROWS if max_rows is None else int(max_rows)
        else:
            offs = np.asarray(row_offsets.numpy() if torch.is_tensor(row_offsets) else row_offsets).astype(np.int64).reshape(-1)
            if len(offs) < 1 or offs[0] != 0 or (np.diff(offs) < 0).any() or offs[-1] != len(rows) or offs[-1] >= 2 ** 31:
                raise ValueError(f"prepare: row_offsets must run from 0 to the {len(rows)} rows given without decreasing")
            d_off = torch.from_numpy(offs.astype(np.int32)).to(dev)
            max_rows = int(np.diff(offs).max()) if len(offs) > 1 else 1
        n = d_off.shape[0] - 1
        d_rows = self._as_dev(rows, torch.float64)
        if d_rows.dim() != 2 or d_rows.shape[1] != 14:
            raise ValueError(f"prepare: rows must be [R, 14], got {tuple(d_rows.shape)}")
        R = d_rows.shape[0]
        d_Pc = self._as_dev(P_cws, torch.float64).reshape(-1, 12)
        if d_Pc.shape[0] != len(ids):
            raise ValueError(f"prepare: {d_Pc.shape[0]} projections for {len(ids)} images")
        d_ids, d_ord = torch.from_numpy(ids).to(dev), torch.from_numpy(order).to(dev)
        ints = torch.empty(4, max(n, 1), device=dev, dtype=torch.int32)      # cls, n_obs, n_valid, status: read back in one copy
        init = torch.empty(n, 5 if rep == 3 else 9, device=dev, dtype=torch.float32)
        half = torch.empty(n, 3, device=dev, dtype=torch.float32) if rep == 3 else None
        pose = torch.empty(n, 7, device=dev, dtype=torch.float64)
        box = torch.empty(n, 8, 3, device=dev, dtype=torch.float64)
        pad = max(R, 1)      # (an empty tensor has no pointer to pass)
        view_img = torch.empty(pad, device=dev, dtype=torch.int32)
        view_row = torch.empty(pad, device=dev, dtype=torch.int32)
        valid = torch.zeros(pad, device=dev, dtype=torch.int32)      # 0 wherever the kernel writes no view: a mask over all R rows
        tgt = torch.empty(pad, 4, device=dev, dtype=torch.float32)
        mask = torch.empty(pad, 4, device=dev, dtype=torch.float32)
        P = torch.empty(pad, 12, device=dev, dtype=torch.float32)
        if n and R:
            with torch.cuda.device(dev), self._lock:
                stream = torch.cuda.current_stream(dev).cuda_stream
                _lib.check(_prepare_entry()(
                    self._h, n, _lib.ptr(d_off), _lib.ptr(d_rows), max(max_rows, 1), len(ids), _lib.ptr(d_ids), _lib.ptr(d_ord), _lib.ptr(d_Pc),
                    float(img_w), float(img_h), float(thr), rep, _lib.ptr(ints[0]), _lib.ptr(ints[1]), _lib.ptr(ints[2]), _lib.ptr(init),
                    _lib.ptr(half), _lib.ptr(pose), _lib.ptr(box), _lib.ptr(ints[3]), _lib.ptr(view_img), _lib.ptr(view_row), _lib.ptr(tgt),
                    _lib.ptr(mask), _lib.ptr(P), _lib.ptr(valid), ctypes.c_void_p(stream)), "odam_sq_prepare_batch")
            h = ints[:, :n].cpu().numpy()
        else:      # no row at all: every track is one without a view
            h = np.zeros((4, n), np.int32)
            h[0], h[3] = -1, PREPARE_NO_VIEW
        return {"cls": h[0], "n_obs": h[1], "n_valid": h[2], "status": h[3], "init": init, "half_dims": half, "pose": pose, "bboxes_dl": box,
                "view_img": view_img[:R], "view_row": view_row[:R], "valid": valid[:R], "tgt": tgt[:R], "mask": mask[:R], "P": P[:R],
                "row_offsets": d_off}

    def prepare_scenes(self, rows, row_offsets, trk_off, img_names_list, P_cws_list, img_hs, img_ws, representation="super_quadric",
                       thr=EDGE_THRESHOLD, max_rows=None):
        """prepare for the tracks of MANY scenes in one launch (include/odam_sq.h, odam_sq_prepare_scenes): every output word is the
        word prepare returns for that scene alone.

        rows, row_offsets, max_rows as prepare takes them, the tracks of all scenes one after the other; trk_off [n_scene + 1] on the
        host: scene s owns tracks trk_off[s] .. trk_off[s + 1] - 1 (an empty scene is legal); img_names_list, P_cws_list, img_hs,
        img_ws: per scene what prepare takes per call -- the image tables are built with frame_tables per scene, as merge_assemble
        builds them, so the same frame id may appear in several scenes.  max_rows may also be one value per scene.  Returns prepare's
        dict ("view_img" is the image index inside the track's scene) with ONE small copy back: cls, n_obs, n_valid, status.

        prepare sizes its launch from the longest track it is given, and the size decides the order of the sums behind a track's yaw;
        so that a scene's words do not depend on what else is in the call, the kernel is told every scene's own size (scene_rows of
        the header): from host offsets the longest track of each scene, as prepare would find it; with a max_rows per scene, those;
        with device offsets and one max_rows (or none), that value for every scene, as prepare(max_rows=...) would take it."""
        dev = self.device
        rep = REPRESENTATIONS[representation]
        to = np.asarray(trk_off.cpu().numpy() if torch.is_tensor(trk_off) else trk_off).astype(np.int64).reshape(-1)
        if len(to) < 1 or to[0] != 0 or (np.diff(to) < 0).any():
            raise ValueError("prepare_scenes: trk_off must start at 0 and not decrease")
        n_scene = len(to) - 1
        if not (len(img_names_list) == len(P_cws_list) == len(img_hs) == len(img_ws) == n_scene):
            raise ValueError(f"prepare_scenes: image names, projections, heights and widths must be given once for each of the {n_scene} scenes")
        if torch.is_tensor(row_offsets) and row_offsets.is_cuda:
            d_off = row_offsets.to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
            offs = None
            n = d_off.shape[0] - 1
            if max_rows is None:
                max_rows = PREPARE_MAX_ROWS
        else:
            offs = np.asarray(row_offsets.numpy() if torch.is_tensor(row_offsets) else row_offsets).astype(np.int64).reshape(-1)
            if len(offs) < 1 or offs[0] != 0 or (np.diff(offs) < 0).any() or offs[-1] != len(rows) or offs[-1] >= 2 ** 31:
                raise ValueError(f"prepare_scenes: row_offsets must run from 0 to the {len(rows)} rows given without decreasing")
            d_off = None
            n = len(offs) - 1
        if int(to[-1]) != n:
            raise ValueError(f"prepare_scenes: trk_off ends at {int(to[-1])}, row_offsets holds {n} tracks")
        if max_rows is None:      # host offsets: every scene as prepare would size it
            lens = np.diff(offs)
            scene_rows = np.array([max(int(lens[to[s]:to[s + 1]].max()), 1) if to[s + 1] > to[s] else 1 for s in range(n_scene)], np.int64)
        else:
            scene_rows = np.broadcast_to(np.asarray(max_rows, np.int64), (n_scene,)).copy()
            scene_rows = np.clip(scene_rows, 1, PREPARE_MAX_ROWS)
        max_rows = int(scene_rows.max()) if n_scene else 1
        d_rows = self._as_dev(rows, torch.float64)
        if d_rows.dim() != 2 or d_rows.shape[1] != 14:
            raise ValueError(f"prepare_scenes: rows must be [R, 14], got {tuple(d_rows.shape)}")
        R = d_rows.shape[0]
        # (img_names_list[s] = None: a scene without an image -- every track of it comes back without a view, status 1)
        tables = [(np.zeros(0, np.int64), np.zeros(0, np.int32)) if names is None else frame_tables(names) for names in img_names_list]
        io = np.zeros(n_scene + 1, np.int64)
        io[1:] = np.cumsum([len(t[0]) for t in tables])
        n_img = int(io[-1])
        ids = np.concatenate([t[0] for t in tables] + [np.zeros(1, np.int64)])      # (one spare word: never a null pointer)
        order = np.concatenate([t[1] for t in tables] + [np.zeros(1, np.int32)])
        wh = np.zeros((n_scene, 2), np.float64)
        wh[:, 0], wh[:, 1] = [float(w) for w in img_ws], [float(h) for h in img_hs]
        # the small tables travel in TWO uploads, whatever the number of scenes: the 32-bit words (offsets, scene sizes, image order) and
        # the 64-bit words (image sizes, frame ids as their bits, and the projections where they are host arrays)
        words = [np.asarray(a, np.int64).astype(np.int32) for a in ((offs,) if offs is not None else ()) + (to, io, scene_rows)] + [order]
        d32 = torch.from_numpy(np.concatenate(words)).to(dev)
        cuts = np.cumsum([0] + [len(a) for a in words])
        parts = [d32[cuts[i]:cuts[i + 1]] for i in range(len(words))]
        if offs is not None:
            d_off, parts = parts[0], parts[1:]
        d_toff, d_ioff, d_srows, d_ord = parts
        host_P = not any(torch.is_tensor(P) for P in P_cws_list)
        Ps = [None if names is None else (np.asarray(P, np.float64).reshape(-1, 12) if host_P else self._as_dev(P, torch.float64).reshape(-1, 12))
              for P, names in zip(P_cws_list, img_names_list)]
        for s, (P, t) in enumerate(zip(Ps, tables)):
            if P is not None and P.shape[0] != len(t[0]):
                raise ValueError(f"prepare_scenes: scene {s} has {P.shape[0]} projections for {len(t[0])} images")
        Ps = [P for P in Ps if P is not None and P.shape[0]]
        quads = [wh.reshape(-1), ids.view(np.float64)] + ([P.reshape(-1) for P in Ps] if host_P else [])
        d64 = torch.from_numpy(np.concatenate(quads)).to(dev)
        d_wh, d_ids = d64[:2 * n_scene], d64[2 * n_scene:2 * n_scene + len(ids)].view(torch.int64)
        if not n_img:
            d_Pc = torch.zeros(1, 12, device=dev, dtype=torch.float64)      # (never a null pointer)
        elif host_P:
            d_Pc = d64[2 * n_scene + len(ids):].reshape(-1, 12)
        else:
            d_Pc = torch.cat(Ps)
        if not n_scene:
            d_wh = torch.zeros(2, device=dev, dtype=torch.float64)
        ints = torch.empty(4, max(n, 1), device=dev, dtype=torch.int32)      # cls, n_obs, n_valid, status: read back in one copy
        init = torch.empty(n, 5 if rep == 3 else 9, device=dev, dtype=torch.float32)
        half = torch.empty(n, 3, device=dev, dtype=torch.float32) if rep == 3 else None
        pose = torch.empty(n, 7, device=dev, dtype=torch.float64)
        box = torch.empty(n, 8, 3, device=dev, dtype=torch.float64)
        pad = max(R, 1)      # (an empty tensor has no pointer to pass)
        view_img = torch.empty(pad, device=dev, dtype=torch.int32)
        view_row = torch.empty(pad, device=dev, dtype=torch.int32)
        valid = torch.zeros(pad, device=dev, dtype=torch.int32)      # 0 wherever the kernel writes no view: a mask over all R rows
        tgt = torch.empty(pad, 4, device=dev, dtype=torch.float32)
        mask = torch.empty(pad, 4, device=dev, dtype=torch.float32)
        P = torch.empty(pad, 12, device=dev, dtype=torch.float32)
        if n and R:
            with torch.cuda.device(dev), self._lock:
                stream = torch.cuda.current_stream(dev).cuda_stream
                _lib.check(_prepare_scenes_entry()(
                    self._h, n, _lib.ptr(d_off), _lib.ptr(d_rows), max(int(max_rows), 1), n_scene, _lib.ptr(d_toff), _lib.ptr(d_ioff), n_img,
                    _lib.ptr(d_ids), _lib.ptr(d_ord), _lib.ptr(d_Pc), _lib.ptr(d_wh), _lib.ptr(d_srows), float(thr), rep, _lib.ptr(ints[0]), _lib.ptr(ints[1]),
                    _lib.ptr(ints[2]), _lib.ptr(init), _lib.ptr(half), _lib.ptr(pose), _lib.ptr(box), _lib.ptr(ints[3]), _lib.ptr(view_img),
                    _lib.ptr(view_row), _lib.ptr(tgt), _lib.ptr(mask), _lib.ptr(P), _lib.ptr(valid), ctypes.c_void_p(stream)),
                    "odam_sq_prepare_scenes")
            h = ints[:, :n].cpu().numpy()
        else:      # no row at all: every track is one without a view
            h = np.zeros((4, n), np.int32)
            h[0], h[3] = -1, PREPARE_NO_VIEW
        return {"cls": h[0], "n_obs": h[1], "n_valid": h[2], "status": h[3], "init": init, "half_dims": half, "pose": pose, "bboxes_dl": box,
                "view_img": view_img[:R], "view_row": view_row[:R], "valid": valid[:R], "tgt": tgt[:R], "mask": mask[:R], "P": P[:R],
                "row_offsets": d_off}

    def _offsets_dev(self, off, dt):
        """offsets given on the host -> (host int64 array, device tensor of dtype dt)"""
        h = np.asarray(off.cpu().numpy() if torch.is_tensor(off) else off).astype(np.int64).reshape(-1)
        if len(h) < 1 or h[0] != 0 or (np.diff(h) < 0).any():
            raise ValueError("offsets must start at 0 and not decrease")
        if dt == torch.int32 and h[-1] >= 2 ** 31:
            raise _lib.OdamError(f"{h[-1]} entries in one call: the offsets are 32-bit")
        return h, torch.from_numpy(h.astype(np.int32 if dt == torch.int32 else np.int64)).to(self.device)

    def merge_cluster(self, iou3d, a_off, pair_off, threshold=MERGE_THRESHOLD):
        """Average-linkage clustering of every scene's tracks in ONE launch (include/odam_merge.h, odam_merge_cluster): what
        sklearn's AgglomerativeClustering(n_clusters=None, distance_threshold=threshold, metric="precomputed", linkage="average")
        answers for the cost 1 - IoU, decision for decision.

        iou3d [n_pairs] float64 on the device as evaluate.iou_scenes(boxes, boxes, cls, cls, gate=2) returns it, a_off / pair_off
        its host offsets.  More than 1024 tracks in a scene raise (ODAM_E_LIMIT) before any launch.  Returns device tensors
        "linkage" [n_tracks, 4] float64 (scene s: rows a_off[s] .. a_off[s+1]-2, scipy's layout), "labels" [n_tracks] int32,
        "n_cluster", "status" [n_scene] int32, "cost" (the kernel's working copy of the costs: after the call no longer the cost
        matrix) and "a_off" on the device.  Nothing is copied back."""
        dev = self.device
        ao, d_aoff = self._offsets_dev(a_off, torch.int32)
        po, d_poff = self._offsets_dev(pair_off, torch.int64)
        n_scene, n_tracks, n_pairs = len(ao) - 1, int(ao[-1]), int(po[-1])
        if len(po) != len(ao) or not np.array_equal(np.diff(po), np.diff(ao) ** 2):
            raise ValueError("merge_cluster: pair_off must hold n_s * n_s words for the n_s tracks of every scene")
        d_iou = self._as_dev(iou3d, torch.float64).reshape(-1)
        if d_iou.shape[0] != n_pairs:
            raise ValueError(f"merge_cluster: {d_iou.shape[0]} IoU words for {n_pairs} pairs")
        max_tracks = int(np.diff(ao).max()) if n_scene else 0
        cost = torch.empty(max(n_pairs, 1), device=dev, dtype=torch.float64)
        link = torch.empty(max(n_tracks, 1), 4, device=dev, dtype=torch.float64)
        labels = torch.empty(max(n_tracks, 1), device=dev, dtype=torch.int32)
        ints = torch.empty(2, max(n_scene, 1), device=dev, dtype=torch.int32)
        if d_iou.shape[0] == 0:
            d_iou = cost
        with torch.cuda.device(dev), self._lock:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(_merge_entry("odam_merge_cluster")(
                self._h, n_scene, _lib.ptr(d_aoff), _lib.ptr(d_poff), n_tracks, n_pairs, max_tracks, _lib.ptr(d_iou), float(threshold),
                _lib.ptr(cost), _lib.ptr(link), _lib.ptr(labels), _lib.ptr(ints[0]), _lib.ptr(ints[1]), ctypes.c_void_p(stream)),
                "odam_merge_cluster")
        return {"linkage": link[:n_tracks], "labels": labels[:n_tracks], "n_cluster": ints[0, :n_scene], "status": ints[1, :n_scene],
                "cost": cost[:n_pairs], "a_off": d_aoff}

    def merge_assemble(self, clusters, a_off, rows, row_offsets, img_names_list, want_rows14=True):
        """The merged tracks of every cluster of every scene (include/odam_merge.h, odam_merge_assemble): merge.py::_merge_cluster on
        the device, three launches.

        clusters: what merge_cluster returned; a_off: its host offsets; rows [R, 14] float64 and row_offsets [n_tracks + 1] as
        prepare takes them, the tracks of all scenes one after the other; img_names_list: the frame ids of every scene's images, all
        different inside a scene.  Returns device tensors "out_off" [n_tracks + 1], "out_src" [R], "out_cls" [n_tracks] int32 and
        "rows14" [R, 14] float64 (None unless want_rows14), of which the first n_out_total + 1, R_out, n_out_total and R_out entries
        are written, and "head" [2 n_scene + 2] int32 = n_out per scene, status per scene, n_out_total, R_out -- ONE small copy
        tells a caller everything it needs to slice the rest.  Nothing is copied back here."""
        dev = self.device
        ao, d_aoff = self._offsets_dev(a_off, torch.int32)
        ro, d_roff = self._offsets_dev(row_offsets, torch.int32)
        n_scene, n_tracks, n_rows = len(ao) - 1, int(ao[-1]), int(ro[-1])
        if len(ro) != n_tracks + 1:
            raise ValueError(f"merge_assemble: {len(ro) - 1} row ranges for {n_tracks} tracks")
        if len(img_names_list) != n_scene:
            raise ValueError("merge_assemble: one list of frame ids per scene")
        d_rows = self._as_dev(rows, torch.float64)
        if d_rows.dim() != 2 or d_rows.shape[1] != 14 or d_rows.shape[0] != n_rows:
            raise ValueError(f"merge_assemble: rows must be [{n_rows}, 14], got {tuple(d_rows.shape)}")
        tables = [frame_tables(names) for names in img_names_list]
        io = np.zeros(n_scene + 1, np.int64)
        io[1:] = np.cumsum([len(t[0]) for t in tables])
        ids = np.concatenate([t[0] for t in tables]) if tables else np.zeros(0, np.int64)
        order = np.concatenate([t[1] for t in tables]) if tables else np.zeros(0, np.int32)
        d_ioff = torch.from_numpy(io.astype(np.int32)).to(dev)
        d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int64)).to(dev) if len(ids) else torch.zeros(1, device=dev, dtype=torch.int64)
        d_ord = torch.from_numpy(np.ascontiguousarray(order, np.int32)).to(dev) if len(ids) else torch.zeros(1, device=dev, dtype=torch.int32)
        max_cand = int(max((ro[ao[s + 1]] - ro[ao[s]] for s in range(n_scene)), default=0))
        scratch = torch.empty(n_rows + 4 * n_tracks + 4, device=dev, dtype=torch.int32)
        out_off = torch.empty(n_tracks + 1, device=dev, dtype=torch.int32)
        out_src = torch.empty(max(n_rows, 1), device=dev, dtype=torch.int32)
        out_cls = torch.empty(max(n_tracks, 1), device=dev, dtype=torch.int32)
        rows14 = torch.empty(max(n_rows, 1), 14, device=dev, dtype=torch.float64) if want_rows14 else None
        head = torch.zeros(2 * n_scene + 2, device=dev, dtype=torch.int32)
        if not d_rows.shape[0]:
            d_rows = torch.zeros(1, 14, device=dev, dtype=torch.float64)
        labels = clusters["labels"] if clusters["labels"].shape[0] else torch.zeros(1, device=dev, dtype=torch.int32)
        with torch.cuda.device(dev), self._lock:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(_merge_entry("odam_merge_assemble")(
                self._h, n_scene, _lib.ptr(d_aoff), n_tracks, _lib.ptr(labels), _lib.ptr(clusters["n_cluster"]),
                _lib.ptr(clusters["status"]), _lib.ptr(d_roff), _lib.ptr(d_rows), n_rows, max_cand, _lib.ptr(d_ioff), _lib.ptr(d_ids),
                _lib.ptr(d_ord), int(io[-1]), _lib.ptr(scratch), _lib.ptr(out_off), _lib.ptr(out_src), _lib.ptr(out_cls),
                _lib.ptr(rows14), _lib.ptr(head[:n_scene]), _lib.ptr(head[n_scene:2 * n_scene]), _lib.ptr(head[2 * n_scene:]),
                ctypes.c_void_p(stream)), "odam_merge_assemble")
        return {"out_off": out_off, "out_src": out_src[:n_rows], "out_cls": out_cls[:n_tracks],
                "rows14": None if rows14 is None else rows14[:n_rows], "head": head}

    def last_launch(self):
        """shape of the newest fit launch (odam_sq_last_launch): grid, threads per workgroup, workgroups per object, longest-first flag"""
        s4 = (ctypes.c_int * 4)()
        _lib.check(_lib.lib().odam_sq_last_launch(self._h, s4), "odam_sq_last_launch")
        return {"grid": s4[0], "threads": s4[1], "split": s4[2], "ordered": bool(s4[3])}

    def fit_dual(self, init5, half_dims, view_counts, P, tgt, mask, n_iters=500, want_loss=False, want_traj=False,
                 check=True):
        """Batched QuadricOptimizer.run (sq_libs.py:194-241): every object through all its steps in ONE launch.

        init5 [n,5] f32 (translate[3], angle, scale_factor); half_dims [n,3] f32 (= dims / 2); view_counts [n];
        P [sumF,3,4]/[sumF,12], tgt, mask [sumF,4] f32.  Returns dict: params [n,5], Q [n,4,4] (device tensors), status
        [n,2] int32 numpy (code, step), loss / traj when asked for.  With check (default) an object whose discriminant
        went negative raises AssertionError, where the reference asserts (sq_libs.py:129,136)."""
        dev = self.device
        n = len(view_counts)
        vc = np.asarray(view_counts, np.int64)
        if n == 0:
            return {"params": torch.zeros(0, 5, device=dev), "Q": torch.zeros(0, 4, 4, device=dev), "status": np.zeros((0, 2), np.int32),
                    "loss": None, "traj": None}
        if vc.min() < 1 or vc.max() > MAX_VIEWS:
            raise _lib.OdamError(f"views per object must be in 1..{MAX_VIEWS}, got {vc.min()}..{vc.max()}")
        as_dev = lambda x, dt: torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(device=dev, dtype=dt).contiguous()
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum(vc)
        d_p0 = as_dev(init5, torch.float32).reshape(n, 5)
        d_h = as_dev(half_dims, torch.float32).reshape(n, 3)
        d_off = as_dev(offs, torch.int32)
        d_P = as_dev(P, torch.float32).reshape(-1, 12)
        d_t = as_dev(tgt, torch.float32).reshape(-1, 4)
        d_m = as_dev(mask, torch.float32).reshape(-1, 4)
        assert d_P.shape[0] == offs[-1] and d_t.shape[0] == offs[-1] and d_m.shape[0] == offs[-1]
        n_iters = int(n_iters)
        out_p = torch.empty(n, 5, device=dev, dtype=torch.float32)
        out_Q = torch.empty(n, 4, 4, device=dev, dtype=torch.float32)
        status = torch.empty(n, 2, device=dev, dtype=torch.int32)
        loss = torch.empty(n, n_iters, device=dev, dtype=torch.float32) if want_loss else None
        traj = torch.empty(n, n_iters, 5, device=dev, dtype=torch.float32) if want_traj else None
        with torch.cuda.device(dev), self._lock:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(_lib.lib().odam_dq_fit_batch(
                self._h, ctypes.c_int(n), _lib.ptr(d_p0), _lib.ptr(d_h), _lib.ptr(d_off), _lib.ptr(d_P), _lib.ptr(d_t), _lib.ptr(d_m),
                ctypes.c_int(n_iters), ctypes.c_int(int(vc.max())), _lib.ptr(out_p), _lib.ptr(out_Q), _lib.ptr(loss), _lib.ptr(traj),
                _lib.ptr(status), ctypes.c_void_p(stream)), "odam_dq_fit_batch")
        st = status.cpu().numpy()
        if check:
            bad = np.flatnonzero(st[:, 0] != 0)
            # the reference's only error path: `assert not torch.isnan(b_x).any()`
            assert len(bad) == 0, "dual-quadric fit: negative discriminant (object, step): %s" % [(int(i), int(st[i, 1])) for i in bad]
        return {"params": out_p, "Q": out_Q, "status": st, "loss": loss, "traj": traj}

    def set_dual_group_waves(self, waves):
        """objects per workgroup of fit_dual's launch (1, 2, 4, 8): scheduling only, results are bit-identical"""
        _lib.check(_lib.lib().odam_dq_set_group_waves(self._h, ctypes.c_int(int(waves))), "odam_dq_set_group_waves")

    def quadric_svd(self, view_counts, P, edges, mask):
        """Batched compute_quadric_svd (sq_libs.py:30-36) over the plane vectors of load_pred_object: the closed-form dual quadric
        of every object from its 2D box edges, float64, ONE launch (include/odam_sq.h, odam_dq_svd_batch).

        view_counts [n]; P [sumF,3,4]/[sumF,12] float64 projections; edges [sumF,4] float64 pixels in the order x_min, x_max,
        y_min, y_max; mask [sumF,4] (0 = edge dropped).  numpy or torch, host or device.  Returns dict: Q [n,4,4] normalised
        (Q[3,3] = -1) and eig [n,3] (smallest, second smallest, largest eigenvalue of A) as float64 device tensors, status [n]
        int32 numpy: 0 an ellipsoid, 1 not one (or no normalisation / sweep limit), 2 nothing computed (fewer than 9 unmasked
        edges or a view count outside 1..MAX_VIEWS; Q and eig NaN)."""
        dev = self.device
        n = len(view_counts)
        vc = np.asarray(view_counts, np.int64).reshape(-1)
        if n == 0:
            return {"Q": torch.zeros(0, 4, 4, device=dev, dtype=torch.float64), "eig": torch.zeros(0, 3, device=dev, dtype=torch.float64),
                    "status": np.zeros(0, np.int32)}
        if vc.min() < 0:
            raise _lib.OdamError(f"views per object must not be negative, got {vc.min()}")
        as_dev = lambda x, dt: torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(device=dev, dtype=dt).contiguous()
        offs = np.zeros(n + 1, np.int64)
        offs[1:] = np.cumsum(vc)
        if offs[-1] >= 2 ** 31:
            raise _lib.OdamError(f"{offs[-1]} views in one call: the offsets are 32-bit")
        d_off = as_dev(offs.astype(np.int32), torch.int32)
        d_P = as_dev(P, torch.float64).reshape(-1, 12)
        d_e = as_dev(edges, torch.float64).reshape(-1, 4)
        d_m = as_dev(mask, torch.float32).reshape(-1, 4)
        assert d_P.shape[0] == offs[-1] and d_e.shape[0] == offs[-1] and d_m.shape[0] == offs[-1]
        out_Q = torch.empty(n, 4, 4, device=dev, dtype=torch.float64)
        out_eig = torch.empty(n, 3, device=dev, dtype=torch.float64)
        status = torch.empty(n, device=dev, dtype=torch.int32)
        # an object outside 1..MAX_VIEWS gets status 2 from the kernel; the launch limit itself must hold
        max_views = int(min(max(int(vc.max()), 1), MAX_VIEWS))
        with torch.cuda.device(dev), self._lock:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(_dq_svd_entry()(self._h, n, _lib.ptr(d_off), _lib.ptr(d_P), _lib.ptr(d_e), _lib.ptr(d_m), max_views,
                                       _lib.ptr(out_Q), _lib.ptr(out_eig), _lib.ptr(status), ctypes.c_void_p(stream)),
                       "odam_dq_svd_batch")
        return {"Q": out_Q, "eig": out_eig, "status": status.cpu().numpy()}

    def _view_rows(self, view_counts):
        """view counts [n] (0 allowed: such an object owns no view) -> device offsets [n + 1] int32, rows in all, max_views of the launch"""
        vc = np.asarray(view_counts, np.int64).reshape(-1)
        if len(vc) and (vc.min() < 0 or vc.max() > MAX_VIEWS):
            raise _lib.OdamError(f"views per object must be in 0..{MAX_VIEWS}, got {vc.min()}..{vc.max()}")
        offs = np.zeros(len(vc) + 1, np.int64)
        offs[1:] = np.cumsum(vc)
        if offs[-1] >= 2 ** 31:
            raise _lib.OdamError(f"{offs[-1]} views in one call: the offsets are 32-bit")
        d_off = torch.from_numpy(offs.astype(np.int32)).to(self.device)
        return d_off, int(offs[-1]), int(max(int(vc.max()) if len(vc) else 1, 1))

    def _as_dev(self, x, dt):
        return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(device=self.device, dtype=dt).contiguous()

    def reproject(self, points, view_counts, P):
        """The 2D box of every object's surface points in every one of its views: the forward half of constraint_2d
        (sq_libs.py:395-413), float32, ONE launch (include/odam_sq.h, odam_sq_reproject_batch).

        points [n, n_pts, 3] (SqFitter.points, or a fit's "points"; n_pts 1..4096); view_counts [n]; P [sumF,3,4]/[sumF,12] as the
        fit saw them.  numpy or torch, host or device.  Returns device tensors: ext [sumF,4] float32 (x_min, x_max, y_min, y_max;
        (1e6, -1e6, 1e6, -1e6) where no point has depth > 0.5) and n_valid [sumF] int32."""
        dev = self.device
        d_pts = self._as_dev(points, torch.float32)
        if d_pts.dim() != 3 or d_pts.shape[2] != 3:
            raise ValueError(f"points must be [n, n_pts, 3], got {tuple(d_pts.shape)}")
        d_off, rows, max_views = self._view_rows(view_counts)
        n = d_off.shape[0] - 1
        d_P = self._as_dev(P, torch.float32).reshape(-1, 12)
        assert d_pts.shape[0] == n and d_P.shape[0] == rows
        ext = torch.empty(rows, 4, device=dev, dtype=torch.float32)
        nvalid = torch.empty(rows, device=dev, dtype=torch.int32)
        if n and rows:      # (objects that own no view at all: nothing to write, and an empty tensor has no pointer to pass)
            with torch.cuda.device(dev), self._lock:
                stream = torch.cuda.current_stream(dev).cuda_stream
                _lib.check(_reproject_entry("odam_sq_reproject_batch")(
                    self._h, n, _lib.ptr(d_pts), int(d_pts.shape[1]), _lib.ptr(d_off), _lib.ptr(d_P), max_views, _lib.ptr(ext),
                    _lib.ptr(nvalid), ctypes.c_void_p(stream)), "odam_sq_reproject_batch")
        return {"ext": ext, "n_valid": nvalid}

    def reproject_dual(self, Q, view_counts, P):
        """DualQuadric.get_bbox (sq_libs.py:289-314) of every object in every one of its views, float64, ONE launch
        (odam_dq_reproject_batch).  Q [n,4,4] (float32 of the iterative fit or float64 of the closed form: computed in float64);
        view_counts [n]; P [sumF,3,4]/[sumF,12] float64.  Returns device tensors: ext [sumF,4] float64 (x_min, x_max, y_min,
        y_max) and status [sumF] int32 (1: negative discriminant or C_22 = 0, the view's extents are NaN)."""
        dev = self.device
        d_Q = self._as_dev(Q, torch.float64).reshape(-1, 16)
        d_off, rows, max_views = self._view_rows(view_counts)
        n = d_off.shape[0] - 1
        d_P = self._as_dev(P, torch.float64).reshape(-1, 12)
        assert d_Q.shape[0] == n and d_P.shape[0] == rows
        ext = torch.empty(rows, 4, device=dev, dtype=torch.float64)
        status = torch.empty(rows, device=dev, dtype=torch.int32)
        if n and rows:
            with torch.cuda.device(dev), self._lock:
                stream = torch.cuda.current_stream(dev).cuda_stream
                _lib.check(_reproject_entry("odam_dq_reproject_batch")(
                    self._h, n, _lib.ptr(d_Q), _lib.ptr(d_off), _lib.ptr(d_P), max_views, _lib.ptr(ext), _lib.ptr(status),
                    ctypes.c_void_p(stream)), "odam_dq_reproject_batch")
        return {"ext": ext, "status": status}

    def reprojection_score(self, ext, bad, view_counts, boxes, mask, img_w, img_h):
        """Predicted edges against detected boxes, per view and per object, ONE launch (odam_reproject_score_f32 / _f64: float64
        when `ext` is float64, else float32).

        ext [sumF,4] from reproject / reproject_dual; bad [sumF] or None (!= 0: a view without prediction -- n_valid == 0, or
        status); view_counts [n]; boxes [sumF,4] detected edges in pixels (x_min, x_max, y_min, y_max); mask [sumF,4].  Returns
        device tensors: residual [sumF,4], iou [sumF]; per object loss_2d, mean_abs_px, mean_iou, min_iou [n] and worst_view,
        n_edges, n_bad [n] int32 (an object without views: NaN, -1, 0, 0)."""
        dev = self.device
        is64 = (ext.dtype == torch.float64) if torch.is_tensor(ext) else (np.asarray(ext).dtype == np.float64)
        dt, name = (torch.float64, "odam_reproject_score_f64") if is64 else (torch.float32, "odam_reproject_score_f32")
        d_ext = self._as_dev(ext, dt).reshape(-1, 4)
        d_off, rows, max_views = self._view_rows(view_counts)
        n = d_off.shape[0] - 1
        d_bad = None if bad is None else self._as_dev(bad, torch.int32).reshape(-1)
        d_box = self._as_dev(boxes, dt).reshape(-1, 4)
        d_m = self._as_dev(mask, torch.float32).reshape(-1, 4)
        assert d_ext.shape[0] == rows and d_box.shape[0] == rows and d_m.shape[0] == rows and (d_bad is None or d_bad.shape[0] == rows)
        res = torch.empty(rows, 4, device=dev, dtype=dt)
        iou = torch.empty(rows, device=dev, dtype=dt)
        obj = torch.empty(n, 4, device=dev, dtype=dt)
        obj_i = torch.empty(n, 3, device=dev, dtype=torch.int32)
        if n and not rows:      # no object owns a view: the rows the kernel would write, without empty tensors' null pointers
            obj.fill_(float("nan"))
            obj_i.zero_()
            obj_i[:, 0] = -1
        elif n:
            with torch.cuda.device(dev), self._lock:
                stream = torch.cuda.current_stream(dev).cuda_stream
                _lib.check(_reproject_entry(name)(
                    self._h, n, _lib.ptr(d_off), _lib.ptr(d_ext), _lib.ptr(d_bad), _lib.ptr(d_box), _lib.ptr(d_m), float(img_w),
                    float(img_h), max_views, _lib.ptr(res), _lib.ptr(iou), _lib.ptr(obj), _lib.ptr(obj_i), ctypes.c_void_p(stream)),
                    name)
        return {"residual": res, "iou": iou, "loss_2d": obj[:, 0], "mean_abs_px": obj[:, 1], "mean_iou": obj[:, 2], "min_iou": obj[:, 3],
                "worst_view": obj_i[:, 0], "n_edges": obj_i[:, 1], "n_bad": obj_i[:, 2]}

    def points(self, params):
        """compute_ellipsoid_points for [n,9] parameter rows -> [n,1000,3] device tensor."""
        dev = self.device
        d_p = torch.as_tensor(np.asarray(params) if not torch.is_tensor(params) else params).to(
            device=dev, dtype=torch.float32).reshape(-1, 9).contiguous()
        n = d_p.shape[0]
        out = torch.empty(n, N_POINTS, 3, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev), self._lock:
            cur = torch.cuda.current_stream(dev)
            stream = cur.cuda_stream
            if self._last is not None and self._last[0] != stream:
                cur.wait_event(self._last[1])
            _lib.check(_lib.lib().odam_sq_points_batch(self._h, ctypes.c_int(n), _lib.ptr(d_p), _lib.ptr(out),
                                                       ctypes.c_void_p(stream)), "odam_sq_points_batch")
            ev = torch.cuda.Event()
            ev.record(cur)
            self._last = (stream, ev)
        return out


def _project_extents(self, params, T_cw, K, on_device=False):
    """[n,9] parameter rows -> [n,4] float64 (x_min, y_min, x_max, y_max) of each surface projected with K @ T_cw[:3]
    (OdamProcess._prepare_tracks, processor.py:181-207), computed on the device"""
    dev = self.device
    d_p = torch.as_tensor(np.asarray(params)).to(device=dev, dtype=torch.float32).reshape(-1, 9).contiguous()
    n = d_p.shape[0]
    out = torch.empty(n, 4, device=dev, dtype=torch.float64)
    cam = np.ascontiguousarray(np.concatenate([np.asarray(T_cw, np.float64)[:3].reshape(-1), np.asarray(K, np.float64)[:3, :3].reshape(-1)]))
    with torch.cuda.device(dev), self._lock:
        cur = torch.cuda.current_stream(dev)
        stream = cur.cuda_stream
        if self._last is not None and self._last[0] != stream:
            cur.wait_event(self._last[1])
        _lib.check(_lib.lib().odam_sq_project_extents(self._h, ctypes.c_int(n), _lib.ptr(d_p), cam.ctypes.data_as(ctypes.c_void_p),
                                                      _lib.ptr(out), ctypes.c_void_p(stream)), "odam_sq_project_extents")
        ev = torch.cuda.Event()
        ev.record(cur)
        self._last = (stream, ev)
    return out if on_device else out.cpu().numpy()


SqFitter.project_extents = _project_extents


def _build_track_windows(self, win, T_cw, K, cam_azi, img_w, img_h):
    """The whole device chain of OdamProcess._prepare_tracks in one native call (include/odam_assoc.h, odam_trackwin_build_tracks):
    parameter rows from the window store's running sums -> surface extents on this fitter -> [T, 79, window] float32 track input
    for the camera T_cw.  `win`: associator.TrackWindows on this fitter's device, in step with the host tracks."""
    dev = self.device
    T = len(win.lengths)
    out = torch.empty(T, 79, win.WINDOW, device=dev, dtype=torch.float32)
    cam = np.ascontiguousarray(np.concatenate([np.asarray(T_cw, np.float64)[:3].reshape(-1), np.asarray(K, np.float64)[:3, :3].reshape(-1)]))
    with torch.cuda.device(dev), self._lock:
        cur = torch.cuda.current_stream(dev)
        stream = cur.cuda_stream
        if self._last is not None and self._last[0] != stream:
            cur.wait_event(self._last[1])
        _lib.check(_lib.lib().odam_trackwin_build_tracks(win._h, self._h, ctypes.c_int(T), cam.ctypes.data_as(ctypes.c_void_p),
                                                         ctypes.c_double(cam_azi), ctypes.c_double(img_w), ctypes.c_double(img_h),
                                                         _lib.ptr(out), ctypes.c_void_p(stream)), "odam_trackwin_build_tracks")
        ev = torch.cuda.Event()
        ev.record(cur)
        self._last = (stream, ev)
    return out


SqFitter.build_track_windows = _build_track_windows


def host_sample(a, e):
    """odam_sq_sample: (a[3], e[2]) -> etas[1000], omegas[1000] float32 (host)."""
    a = np.ascontiguousarray(a, np.float32)
    e = np.ascontiguousarray(e, np.float32)
    et = np.zeros(N_POINTS, np.float32)
    om = np.zeros(N_POINTS, np.float32)
    fp = _lib.c_float_p
    _lib.check(_lib.lib().odam_sq_sample(a.ctypes.data_as(fp), e.ctypes.data_as(fp), et.ctypes.data_as(fp),
                                         om.ctypes.data_as(fp)), "odam_sq_sample")
    return et, om


def init_dual(translate, angle, dims):
    """QuadricOptimizer.__init__ (sq_libs.py:41-58): (translate[3], angle, scale_factor = 1) and h = dims / 2, float32."""
    init5 = np.concatenate([np.asarray(translate, np.float64).reshape(3), [float(angle)], [1.0]]).astype(np.float32)
    return init5, (np.asarray(dims, np.float64).reshape(3) / 2).astype(np.float32)


def dual_params2mat(p5, half_dims):
    """QuadricOptimizer.params2mat (sq_libs.py:68-78) of a float32 state, for objects that were not fitted (Q_init): the
    reference's own operations -- float32 (T @ diag) @ T.T by the host BLAS."""
    p = np.asarray(p5, np.float32)
    a = (p[4] * np.asarray(half_dims, np.float32)) ** 2
    c, s = np.cos(p[3]), np.sin(p[3])
    T = np.array([[c, -s, 0, p[0]], [s, c, 0, p[1]], [0, 0, 1, p[2]], [0, 0, 0, 1]], np.float32)
    return (T @ np.diag(np.concatenate([a, [np.float32(-1)]]).astype(np.float32)) @ T.T).astype(np.float32)


class DualQuadric:
    """The reference's DualQuadric (sq_libs.py:244-348) over a 4x4 float32 matrix.  Host code: get_srt's eigenvector bits are
    LAPACK's (scipy.linalg.eig, the routine the reference calls), so it stays on scipy rather than in the native library."""

    def __init__(self, Q):
        self.Q = np.asarray(Q)

    def projection(self, P, if_vectorize=False):
        return P @ self.Q @ P.T

    def get_srt(self):      # sq_libs.py:257-280
        import scipy.linalg
        t_wo = -self.Q[:3, 3:]
        A = self.Q[:3, :3] + t_wo @ t_wo.T
        scale, R_wo = scipy.linalg.eig(A)
        scale = scale.astype(np.float32)      # (drops a zero imaginary part, as upstream)
        if np.linalg.det(R_wo) < 0:
            R_wo *= -1
        is_ellipsoid = not (scale < 0).any()
        scale = np.abs(scale)
        return scale, R_wo, t_wo, is_ellipsoid

    def transform(self, T_cw):
        return T_cw @ self.Q @ T_cw.T

    def get_bbox(self, P, if_vectorize=False, line_form=False):      # sq_libs.py:289-314
        C = self.projection(P, if_vectorize)
        with np.errstate(invalid="ignore"):
            b_x = np.sqrt(4 * C[0, 2] ** 2 - 4 * C[0, 0] * C[2, 2])
            b_y = np.sqrt(4 * C[1, 2] ** 2 - 4 * C[1, 1] * C[2, 2])
        x_0, x_1 = 0.5 / C[2, 2] * (2 * C[0, 2] + b_x), 0.5 / C[2, 2] * (2 * C[0, 2] - b_x)
        y_0, y_1 = 0.5 / C[2, 2] * (2 * C[1, 2] + b_y), 0.5 / C[2, 2] * (2 * C[1, 2] - b_y)
        x_min, x_max, y_min, y_max = min(x_0, x_1), max(x_0, x_1), min(y_0, y_1), max(y_0, y_1)
        if line_form:
            return [np.array([1, 0, -x_min]), np.array([0, 1, -y_min]), np.array([1, 0, -x_max]), np.array([0, 1, -y_max])]
        return np.array([x_min, y_min, x_max, y_max])

    def compute_ellipsoid_points(self, use_numpy=None):      # sq_libs.py:316-348
        axes, R, centre, is_ellipsoid = self.get_srt()
        axes = np.sqrt(axes)
        centre = centre.flatten()
        side = 50
        u = np.linspace(0, 2 * np.pi, side)
        v = np.linspace(0, np.pi, side)
        x = axes[0] * np.outer(np.cos(u), np.sin(v))
        y = axes[1] * np.outer(np.sin(u), np.sin(v))
        z = axes[2] * np.outer(np.ones_like(u), np.cos(v))
        x, y, z = np.tensordot(R, np.vstack((x, y, z)).reshape((3, side, side)), axes=1)
        pts = np.stack([(x + centre[0]).reshape(-1), (y + centre[1]).reshape(-1), (z + centre[2]).reshape(-1)], axis=1)
        return pts.astype(np.float32), is_ellipsoid
