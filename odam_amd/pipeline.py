"""One scene through the whole chain on N ranks -- what the reference's driver does on one process
(likojack/ODAM src/scripts/run_processor.py:70-83):

    for frame: process_frame(rgb, frame_id, T_wc)        # detect -> associate -> attach   (src/processor.py:306-345)
    out = optim_process(tracks); tracks = merge_process(out); out = optim_process(tracks)

with the two data-parallel halves sharded and everything in between replayed identically on every rank:

    chunk of frames -> each rank detects ITS frames of the chunk -> all-gather of the detection blocks (collective #1)
                    -> every rank replays process_frame over the chunk's frames in order (association is sequential)
    tracks (identical on every rank) -> object_shard by observation count -> each rank fits ITS objects
                    -> all-gather of parameters + boxes (collective #2) -> every rank holds the full result dict
    merge_process on every rank (deterministic host code) -> second sharded fit pass.

`run_scene` is the product entry; the ranks are the processes of the current torch.distributed group (one per GPU, backend
"nccl" = RCCL; "gloo" in the tests), or a world of one without a group.  The result dict has the reference's pickle layout
(run_processor.py:85-92) on EVERY rank.  Detection rows travel as float32 -- they are float32 values widened to float64 by
run_detector (processor.py:276-288), so nothing is lost -- and float64 boxes travel bit for bit (as pairs of 32-bit words): an
N-rank run returns what the one-rank run returns, bit for bit, when the detector's kernel choice does not depend on how many
frames a rank holds (odam_config key cg.pin = 1; otherwise to the fp32 reorder noise of different tile shapes, ~1e-5).
"""
import numpy as np

from . import multi_view, parallel

# one fitted object on the wire: 9 parameters | fitted flag | class | bboxes_qc 8x3 float64 | bboxes_dl 8x3 float64 (as float32 words)
_FIT_COLS = 9 + 1 + 1 + 48 + 48


def _f64_words(a):
    """float64 [n, 24] -> float32 [n, 48] holding the same bytes (a gather moves bytes: the values arrive bit for bit)"""
    return np.ascontiguousarray(a, np.float64).reshape(len(a), 24).view(np.float32)


def detect_gathered(detect, first, end, device=None, force=False, packed=False):
    """Frames first .. end-1 of the scene: this rank detects its contiguous share (parallel.frame_shard of the span), the
    blocks are all-gathered, every rank returns the rows of ALL frames of the span in frame order (list of [n, 79] float64).
    `detect(f0, f1)` -> list (per frame) of [n, 79] rows for scene frames f0 .. f1-1; with `packed`, the packed block and
    counts themselves (OdamProcess.detect_frames_packed: device tensors that go straight into the gather)."""
    rank, ws = parallel.world()
    n = end - first
    s, e = parallel.frame_shard(n, rank, ws)
    if packed and e > s:
        blk, cnt = detect(first + s, first + e)
        blk, cnt = parallel.allgather_detections(blk, cnt, n, device, force=force)
        return parallel.unpack_detections(blk, cnt)
    rows = detect(first + s, first + e) if e > s else []
    blk, cnt = parallel.pack_detections(rows)
    blk, cnt = parallel.allgather_detections(blk, cnt, n, device, force=force)
    return parallel.unpack_detections(blk, cnt)


def sharded_optim(proc, tracks, device=None, force=False):
    """optim_process (src/scripts/run_multi_view.py:22-76) with the objects dealt over the ranks: each rank fits its share
    (longest tracks first, round-robin), one all-gather brings parameters and boxes of every object to every rank.
    Returns the reference's dict {"tracks", "bboxes_qc", "bboxes_dl", "quadrics"} for ALL objects."""
    rank, ws = parallel.world()
    n = len(tracks)
    owners = [parallel.object_shard([len(t) for t in tracks], r, ws) for r in range(ws)]
    mine = owners[rank]
    local = np.zeros((len(mine), _FIT_COLS), np.float32)
    if mine:
        out = proc.optim_process_params([tracks[i] for i in mine])
        local[:, :9] = out["params"]
        local[:, 9] = out["fitted"]
        local[:, 10] = [q.obj_class for q in out["quadrics"]]
        local[:, 11:59] = _f64_words(np.asarray(out["bboxes_qc"], np.float64))
        local[:, 59:107] = _f64_words(np.asarray(out["bboxes_dl"], np.float64))
        mine_quadrics = dict(zip(mine, out["quadrics"]))
    else:
        mine_quadrics = {}
    rows = parallel.allgather_rows(local, n, owners, device, force=force)
    fitter = proc._fitter()
    qc = np.ascontiguousarray(rows[:, 11:59]).view(np.float64).reshape(n, 8, 3)
    dl = np.ascontiguousarray(rows[:, 59:107]).view(np.float64).reshape(n, 8, 3)
    quadrics = []
    for i in range(n):
        # the objects this rank fitted keep their sampled surface; the others re-sample it from the parameters on demand
        # (compute_ellipsoid_points: the same sampler and surface code on the same nine floats)
        quadrics.append(mine_quadrics.get(i) or multi_view.SuperQuadric(rows[i, :9], int(rows[i, 10]), None, fitter))
    return {"tracks": tracks, "bboxes_qc": [qc[i] for i in range(n)], "bboxes_dl": [dl[i] for i in range(n)],
            "quadrics": quadrics, "params": rows[:, :9].copy(), "fitted": rows[:, 9] != 0}


def _associate(proc, frame_ids, T_wcs, c0, rows):
    """the sequential association loop (src/processor.py:306-345) over the frames c0 ... of a chunk whose detections are at hand: as one
    process_frames call where the process object has it (the host's work then sits under the device's, processor.py), frame by frame otherwise"""
    if hasattr(proc, "process_frames"):
        n = len(rows)
        proc.process_frames([int(frame_ids[c0 + i]) for i in range(n)], [T_wcs[c0 + i] for i in range(n)], rows)
    else:
        for i, r in enumerate(rows):
            proc.process_frame(None, int(frame_ids[c0 + i]), T_wcs[c0 + i], detections=r)


def map_scene(proc, tracks=None, resident_rows=False, device_merge=False, stages=None, loaded=False):
    """The back end of run_scene on ONE rank: fit -> merge -> fit over `tracks` (default: proc.tracks), returning the second
    optim_process dict (with "params" and "fitted") and filling `stages` with the seconds of fit1, merge and fit2 and the first pass's dict.

    resident_rows  the tracks' rows go to the device ONCE (track_store.TrackRows.load) and stay there through the chain: pass 1 is fitted
              from the store's block, merge.merge_packed assembles from the same block and leaves the merged rows on the device, the
              store adopts them, pass 2 is fitted from the adopted block, and the merged host tracks (merge.tracks_from_packed) are gathered
              while pass 2 runs -- no concatenate and no upload of track rows after the load; the device prelude and the device merge
              are implied, and the results are theirs, bit for bit.  A list the store refuses takes the path below; a scene the device
              merge refuses (merge._device_scene) takes the host merge, followed by a load of the merged tracks.
    loaded    with resident_rows: the store (proc._rows) holds the tracks' rows already -- a sequence fed by
              OdamProcess.track_frames_packed(resident=True) -- so nothing is loaded: its block is taken as it stands, and the host list
              (TrackRows.host_tracks) is downloaded under the first pass, for the result dicts and the merged host tracks.  `tracks` is
              not used.  The store holds the MERGED tracks afterwards, so the sequence's view of it ends here: proc.tracks is the
              unmerged host list from then on.
    device_merge   without resident_rows: proc.merge_process(out, on_device=True), as in run_scene."""
    import time
    from . import merge
    if loaded and not (resident_rows and getattr(proc, "_rows", None) is not None):
        raise ValueError("map_scene(loaded=True) needs resident_rows=True and a row store that was fed (track_frames_packed(resident=True))")
    release = getattr(proc, "_release_store", lambda: None)
    t = {}
    store = block = None
    if loaded:
        store = proc._rows
        block, tracks = store.packed(), store.host_tracks
    else:
        tracks = proc.tracks if tracks is None else tracks
    if resident_rows and not loaded:
        release()      # the store is loaded below: a sequence that was a view of it keeps its list
        if proc._rows is None:
            from .track_store import TrackRows
            proc._rows = TrackRows(proc._fitter())
        store = proc._rows
        if store.load(tracks) is not None:
            block = store.packed()
    s0 = time.perf_counter()
    if block is None:
        out = proc.optim_process_params(tracks)
        s1 = time.perf_counter()
        merged = proc.merge_process(out, on_device=True) if device_merge else proc.merge_process(out)
        s2 = time.perf_counter()
        out2 = proc.optim_process_params(merged)
    else:
        out = proc.optim_process(tracks, return_params=True, rows=block)
        release()      # (loaded: the list was downloaded under the fit; the store is about to hold other rows)
        s1 = time.perf_counter()
        proc._refine_state = None      # keyed by track index (OdamProcess.merge_process drops it too)
        packed = merge.merge_packed(out, proc.usable_frames, fitter=proc._fitter(), rows=block)
        if packed is None:
            merged = proc.merge_process(out)
            block2 = store.packed() if store.load(merged) is not None else None
            s2 = time.perf_counter()
            out2 = proc.optim_process(merged, return_params=True, rows=block2) if block2 is not None else proc.optim_process_params(merged)
        else:
            store.adopt(packed)
            s2 = time.perf_counter()
            out2 = proc.optim_process(lambda: merge.tracks_from_packed(packed, out), return_params=True, rows=store.packed())
    t.update(fit1=s1 - s0, merge=s2 - s1, fit2=time.perf_counter() - s2)
    if stages is not None:
        stages.update(t)
        stages["first_pass"] = out
    return out2


def _shared_settings(procs):
    """what the process objects of map_scenes must have in common, read without touching the device: (fit settings, fitter key)"""
    first = None
    for i, p in enumerate(procs):
        fit = p.fit_settings() if hasattr(p, "fit_settings") else None
        if fit is None:
            raise ValueError(f"map_scenes: process {i} does not say how it fits (OdamProcess.fit_settings)")
        if fit["representation"] == "dual_quadric":
            raise ValueError(f'map_scenes: process {i} fits "dual_quadric", which is not fitted over scenes (map_scene takes it)')
        dev = str(getattr(getattr(p, "detector", None), "device", "cuda:0"))
        f = p.fitter if p.fitter is not None else multi_view._DEFAULT_FITTER.get(dev, ("default fitter", dev))
        if first is None:
            first = (fit, f)
        elif fit != first[0]:
            raise ValueError(f"map_scenes: process {i} fits with {fit}, process 0 with {first[0]}: representation, prior, steps and n_views are shared")
        elif f is not first[1] and f != first[1]:
            raise ValueError(f"map_scenes: process {i} has another fitter (or device) than process 0: one launch runs on one SqFitter")
    return first


def map_scenes(procs, loaded=False, stages=None):
    """map_scene(proc, resident_rows=True, loaded=loaded) for every process object of the list, in the launches of ONE scene:
    the rows of all stores as one block (track_store.pack_scenes), pass 1 as one multi_view.optim_process_scenes, the merge as one
    merge.merge_packed_scenes, the stores' adoption of the merged rows with one copy back (track_store.adopt_scenes), pass 2 as one
    optim_process_scenes.  Returns the list of second-pass dicts, each the bits of the single-scene call.

    All procs share one fitter (hence device), representation, prior setting, step count and n_views -- ValueError before any device
    work otherwise, and for "dual_quadric".  A scene leaves the batch only for a reason map_scene itself has: its store refuses the
    list, a prelude status, a scene merge._device_scene refuses, a merge status -- decided from the copies the batch makes anyway.  One
    that leaves before or at the first prelude goes through map_scene; one that leaves at the merge (or at the second prelude) completes
    its second pass in map_scene's own code path; both after the batch.
    stages: fit1, merge, fit2 (seconds of the batch), first_pass (list of dicts), batched (indices that went through all three steps in
    the batch), single (the others)."""
    import time
    from . import merge, track_store
    procs = list(procs)
    n = len(procs)
    if n == 0:
        if stages is not None:
            stages.update(fit1=0.0, merge=0.0, fit2=0.0, first_pass=[], batched=[], single=[])
        return []
    fit, _ = _shared_settings(procs)
    if loaded:
        for i, p in enumerate(procs):
            if getattr(p, "_rows", None) is None:
                raise ValueError(f"map_scenes(loaded=True): process {i} has no row store that was fed (track_frames_packed(resident=True))")
    fitter = procs[0]._fitter()
    release = [getattr(p, "_release_store", lambda: None) for p in procs]
    stores, tracks, alone = [None] * n, [None] * n, []
    for i, p in enumerate(procs):
        if loaded:
            stores[i], tracks[i] = p._rows, p._rows.host_tracks
            continue
        release[i]()
        if p._rows is None:
            p._rows = track_store.TrackRows(fitter)
        tracks[i] = p.tracks
        if p._rows.load(tracks[i]) is None:
            alone.append(i)      # map_scene's host path
        else:
            stores[i] = p._rows
    first, second = [None] * n, [None] * n
    meta = lambda p: {"img_names": p.usable_frames, "P_cws": p.P_cws, "img_h": p.sequence_meta.img_h, "img_w": p.sequence_meta.img_w}
    args = (fit["representation"], fit["prior"], fit["n_iters"], fit["n_views"])

    s0 = time.perf_counter()
    ids = [i for i in range(n) if stores[i] is not None]
    if ids:
        outs, left = multi_view.optim_process_scenes([dict(meta(procs[i]), tracks=tracks[i]) for i in ids],
                                                     track_store.pack_scenes([stores[i] for i in ids]), *args, fitter=fitter)
        for k, i in enumerate(ids):
            if k in left:
                alone.append(i)
            else:
                first[i] = outs[k]
                release[i]()      # (loaded: the list was downloaded under the fit; the store is about to hold other rows)
                procs[i]._refine_state = None
        ids = [i for k, i in enumerate(ids) if k not in left]
    s1 = time.perf_counter()

    finish = {}      # scenes that complete their second pass as map_scene does: index -> callable
    block = None
    if ids:
        block, per = merge.merge_packed_scenes([first[i] for i in ids], [procs[i].usable_frames for i in ids], fitter=fitter,
                                               rows=track_store.pack_scenes([stores[i] for i in ids]))
        went = [i for k, i in enumerate(ids) if per[k] is not None]
        for k, i in enumerate(ids):
            if per[k] is None:
                finish[i] = lambda i=i: _second_pass_alone(procs[i], stores[i], first[i])
        if went:
            track_store.adopt_scenes([stores[i] if per[k] is not None else None for k, i in enumerate(ids)], block)
        order, ids = ids, went
    s2 = time.perf_counter()

    if ids:
        host = {}

        def merged_tracks(i):      # the merged host tracks of all scenes: ONE copy back, made under pass 2
            if not host:
                host.update(zip(order, merge.tracks_from_packed_scenes(block, [first[j] for j in order])))
            return host[i]
        outs, left = multi_view.optim_process_scenes([dict(meta(procs[i]), tracks=lambda i=i: merged_tracks(i)) for i in ids],
                                                     track_store.pack_scenes([stores[i] for i in ids]), *args, fitter=fitter)
        for k, i in enumerate(ids):
            if k in left:      # optim_process(rows=...) falls back on the host list there
                finish[i] = lambda i=i: procs[i].optim_process(lambda: merged_tracks(i), return_params=True, rows=stores[i].packed())
            else:
                second[i] = outs[k]
        ids = [i for k, i in enumerate(ids) if k not in left]
    s3 = time.perf_counter()

    for i, f in finish.items():
        second[i] = f()
    for i in alone:
        st = {}
        second[i] = map_scene(procs[i], None if loaded else tracks[i], resident_rows=True, stages=st, loaded=loaded)
        first[i] = st["first_pass"]
    if stages is not None:
        stages.update(fit1=s1 - s0, merge=s2 - s1, fit2=s3 - s2, first_pass=first, batched=sorted(ids),
                      single=sorted(set(range(n)) - set(ids)))
    return second


def _second_pass_alone(proc, store, out):
    """map_scene's own lines for a scene the device merge does not take: the host merge, a load of the merged tracks, pass 2"""
    merged = proc.merge_process(out)
    block2 = store.packed() if store.load(merged) is not None else None
    return proc.optim_process(merged, return_params=True, rows=block2) if block2 is not None else proc.optim_process_params(merged)


def run_scene(proc, n_frames, frame_ids, T_wcs, detect=None, frames=None, chunk=0, device=None, force=False, stages=None, overlap=None,
              device_select=False, device_merge=False):
    """The driver loop of run_processor.py:70-83 for one scene on the ranks of the current process group.

    proc      OdamProcess after init_sequence (its detector is used unless `detect` is given; its associator and fitter always)
    detect    optional callable (f0, f1) -> per-frame [n, 79] rows for scene frames f0 .. f1-1 (e.g. a batched, device-resident
              path); default: proc.detect_frames over frames[f0:f1]
    chunk     frames per all-gather (0 = the whole scene in one): association of a chunk starts when its detections arrive
    stages    optional dict that receives wall-clock seconds per stage (detect + gather, associate, fit 1, merge, fit 2)
    overlap   detection + all-gather of chunk i + 1 run on a worker thread while this thread replays process_frame over chunk i
              ("chunking lets association overlap detection"; src/processor.py:306-345 is the loop that is replicated).
              None = on in a world of more than one rank with more than one chunk: there a rank's share of a chunk's detection is
              1 / N of it while the replicated association is not, so the chain runs at max(associate, detect / N) instead of their
              sum; on ONE GPU the association's short launches wait behind the detector's queued ones (profiles/
              r4_experiments_not_kept.txt #12, #13) and the overlap returns nothing.  Only the worker issues collectives while it
              runs, in chunk order on every rank; results are identical with and without (the same calls on the same data).
    device_select  with the default `detect` only: a rank's share goes through proc.detect_frames_packed -- threshold, NMS and the rows
              on the device -- and the packed block straight into the gather; the same detections, bit for bit.  Frames of one size.
    device_merge   the track merge between the two fit passes clusters and assembles on the device too (proc.merge_process(out,
              on_device=True)): the same merged tracks, decision for decision.
    Returns the second optim_process dict (what the reference pickles), identical on every rank; proc.tracks holds the
    unmerged tracks."""
    import sys
    import time
    packed = bool(device_select) and detect is None
    if detect is None:
        if frames is None:
            raise ValueError("run_scene: give `frames` or a `detect` callable")

        def detect(f0, f1):
            return [np.asarray(r, np.float64).reshape(-1, 79) for r in proc.detect_frames(list(frames[f0:f1]), list(frame_ids[f0:f1]))]
        if packed:
            def detect(f0, f1):      # noqa: F811
                return proc.detect_frames_packed(list(frames[f0:f1]), list(frame_ids[f0:f1]))
    t = {"detect_gather": 0.0, "associate": 0.0}
    spans = parallel.chunk_spans(n_frames, chunk or n_frames)
    if overlap is None:
        overlap = parallel.world()[1] > 1 and len(spans) > 1
    if overlap and len(spans) > 1:
        import queue
        import threading
        import torch
        q = queue.Queue(maxsize=2)      # at most two chunks of detections ahead of the association loop
        cancel = threading.Event()
        # HIP's current device is per THREAD and a new thread starts on device 0: resolve the device here, on the caller's thread, to a
        # full name ('cuda:N') and make it the worker's current device -- with device=None, rank r's worker would otherwise resolve
        # 'cuda' (and parallel._dev_key(None)) to GPU 0 and put its collective tensors there
        if device is None:
            wdev = parallel._dev_key(None) if (torch.cuda.is_available() and torch.cuda.is_initialized()) else None
        else:
            wdev = str(device) if str(device) == "cpu" else parallel._dev_key(device)

        def put(item):
            while not cancel.is_set():
                try:
                    q.put(item, timeout=0.1)
                    return True
                except queue.Full:
                    pass
            return False

        def produce():
            try:
                if wdev is not None and wdev != "cpu":
                    torch.cuda.set_device(torch.device(wdev))
                for c0, c1 in spans:
                    if cancel.is_set():      # the consumer failed: issue no further collective from this rank
                        return
                    s0 = time.perf_counter()
                    rows = detect_gathered(detect, c0, c1, device, force, packed)
                    if not put((c0, rows, time.perf_counter() - s0)):
                        return
                put(None)
            except BaseException as e:      # noqa: BLE001 -- handed to the consumer, which re-raises it
                put(e)

        th = threading.Thread(target=produce, name="odam-detect", daemon=True)
        th.start()
        waited = 0.0
        try:
            while True:
                s0 = time.perf_counter()
                item = q.get()
                waited += time.perf_counter() - s0
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                c0, rows, dt_detect = item
                s1 = time.perf_counter()
                _associate(proc, frame_ids, T_wcs, c0, rows)
                t["associate"] += time.perf_counter() - s1
                t["detect_gather"] += dt_detect
        finally:
            # on an exception (here or in the producer) the worker must not keep issuing collectives on this rank alone, nor stay blocked on
            # a full queue: tell it to stop, make room, wait for it.  (A collective it is INSIDE completes only if the peers reach it too;
            # the join is bounded so that this rank's exception surfaces either way.)
            cancel.set()
            try:
                while True:
                    q.get_nowait()
            except queue.Empty:
                pass
            th.join(timeout=None if sys.exc_info()[0] is None else 30.0)
        t["overlapped"] = True
        t["associate_waited_for_detections"] = waited      # what the association loop did NOT hide
    else:
        for c0, c1 in spans:
            s0 = time.perf_counter()
            rows = detect_gathered(detect, c0, c1, device, force, packed)
            s1 = time.perf_counter()
            _associate(proc, frame_ids, T_wcs, c0, rows)
            t["detect_gather"] += s1 - s0
            t["associate"] += time.perf_counter() - s1
    s0 = time.perf_counter()
    out = sharded_optim(proc, proc.tracks, device, force)
    s1 = time.perf_counter()
    merged = proc.merge_process(out, on_device=True) if device_merge else proc.merge_process(out)
    s2 = time.perf_counter()
    out2 = sharded_optim(proc, merged, device, force)
    t.update(fit1=s1 - s0, merge=s2 - s1, fit2=time.perf_counter() - s2)
    if stages is not None:
        stages.update(t)
        stages["first_pass"] = out
    return out2
