"""The detector's validation loss on the device: the reference's HungarianMatcher (src/models/matcher.py:11-82) and SetCriterion
(src/models/detr.py:258-481, without masks and gradients) under their own names and argument order, over the entry points of
include/odam_loss.h (csrc/det_loss.hip).  With "aux_outputs" among the outputs (Detector(..., aux=True)) every decoder layer is
matched and scored in the same few launches, and the total is the one of the model's training log (build(cfg) with aux_loss).

    criterion = odam_amd.criterion.build(cfg)                  # or SetCriterion(num_classes, HungarianMatcher(...), weight_dict, eos_coef, losses)
    losses = criterion(det(frames), targets)                   # {"loss_ce": 0-d tensor, "class_error": ..., ...}
    total = criterion.total(losses)                            # sum(losses[k] * criterion.weight_dict[k])

`outputs` is what Detector.__call__ returns (device tensors; "pred_obj_features", "_hw" and any other key are ignored) or a dict
of host arrays; `targets` the reference's list of {"objects": [n, W]} (tensors or arrays, W >= 12: 0 label, 1:5 box cx cy w h,
5:8 size, 8:10 offset, W-2 depth, W-1 angle bin).  The cost matrix, the assignment and every sum stay on the device: one block of
ODAM_LOSS_N_ENTRIES float64 and the status words comes back to the host per call (and the indices, when the matcher is called
directly).  There is no host path: without the library's kernels every call raises."""
import ctypes

import numpy as np
import torch

from . import _lib

LOSS_NAMES = ("labels", "boxes", "cardinality", "size", "angle", "offset", "depth")
# out_table of odam_detr_criterion, in order (include/odam_loss.h)
TABLE_KEYS = ("loss_ce", "class_error", "cardinality_error", "loss_bbox", "loss_giou", "loss_size", "loss_offset", "loss_depth",
              "loss_angle", "total")
# out_partial, per frame
PARTIAL_KEYS = ("sum_w_nll", "sum_w", "n_correct", "n_matched", "cardinality_abs", "sum_bbox", "sum_giou", "sum_size", "sum_offset",
                "sum_depth", "sum_angle")
# the order of the `weights` argument, which is also the order total() adds in
WEIGHT_KEYS = ("loss_ce", "loss_bbox", "loss_giou", "loss_size", "loss_offset", "loss_depth", "loss_angle")
KEYS_OF_LOSS = {"labels": ("loss_ce", "class_error"), "cardinality": ("cardinality_error",), "boxes": ("loss_bbox", "loss_giou"),
                "size": ("loss_size",), "angle": ("loss_angle",), "offset": ("loss_offset",), "depth": ("loss_depth",)}
LSAP_MAX_SMALL, LSAP_MAX_LARGE = 32, 128
ST_DEGENERATE, ST_CLASS, ST_OFFSETS = 1, 2, 4
MIN_W = 12

_P, _I, _L, _F, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double
LOSS_ARGTYPES = {
    "odam_detr_match_cost": [_P, _P, _I, _I, _I, _P, _P, _I, _I, _F, _F, _F, _P, _P, _P],
    "odam_lsap_batch": [_P, _L, _P, _P, _P, _I, _I, _I, _P, _L, _P, _P, _P, _P],
    "odam_detr_criterion": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _P, _D, _F, _P, _P, _P, _P, _P],
    "odam_detr_match_cost_layers": [_P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _F, _F, _F, _P, _P, _P],
    "odam_detr_criterion_layers": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _I, _P, _D, _F, _P, _P, _P, _P, _P],
}
_OUT_KEYS = ("pred_logits", "pred_boxes", "pred_angle", "pred_offset", "pred_size", "pred_depth")
_OUT_LAST = {"pred_boxes": 4, "pred_offset": 2, "pred_size": 3, "pred_depth": 1}


def _entry(name):
    f = getattr(_lib.lib(), name)
    if f.argtypes is None:
        f.argtypes, f.restype = LOSS_ARGTYPES[name], ctypes.c_int
    return f


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _f32(x, dev):
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


class _Staged:
    """the device view of one (outputs, targets) pair: the six output tensors, the target block and its offsets"""

    def __init__(self, outputs, targets, keys=_OUT_KEYS, device=None):
        if "pred_logits" not in outputs or "pred_boxes" not in outputs:
            raise KeyError("outputs need pred_logits and pred_boxes")
        first = outputs["pred_logits"]
        if device is None:
            device = first.device if torch.is_tensor(first) and first.is_cuda else torch.device("cuda:0")
        self.dev = dev = torch.device(device)
        # every shape is checked before anything is moved to the device
        for k in keys:
            if k not in outputs:
                raise KeyError(f"outputs have no {k!r}")
        shape = {k: tuple(int(v) for v in outputs[k].shape) for k in keys}
        if len(shape["pred_logits"]) != 3 or shape["pred_logits"][2] < 2:
            raise ValueError("pred_logits must be [B, Q, classes + 1]")
        self.B, self.Q, self.n_logit = shape["pred_logits"]
        for k, last in _OUT_LAST.items():
            if k in shape and shape[k] != (self.B, self.Q, last):
                raise ValueError(f"{k} must be [{self.B}, {self.Q}, {last}], got {shape[k]}")
        if "pred_angle" in shape and (len(shape["pred_angle"]) != 3 or shape["pred_angle"][:2] != (self.B, self.Q) or shape["pred_angle"][2] < 1):
            raise ValueError("pred_angle must be [B, Q, bins]")
        if len(targets) != self.B:
            raise ValueError(f"{len(targets)} targets for {self.B} frames")
        oshape = [tuple(int(v) for v in t["objects"].shape) for t in targets]
        if any(len(o) != 2 for o in oshape):
            raise ValueError('target "objects" must be [n, W]')
        widths = {o[1] for o in oshape}
        if len(widths) != 1:
            raise ValueError(f'target "objects" of one batch must share their width, got {sorted(widths)}')
        self.W = widths.pop()
        if self.W < MIN_W:
            raise ValueError(f'target "objects" need W >= {MIN_W} columns (label, box, size, offset, ..., depth, angle bin), got {self.W}')
        self.t = {k: _f32(outputs[k], dev) for k in keys}
        objs = [_f32(t["objects"], dev) for t in targets]
        self.sizes = [int(o.shape[0]) for o in objs]
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.n_obj = int(self.off[-1])
        # one row of padding keeps the pointer valid when no frame has a target; it is owned by no frame and never read
        self.objects = torch.cat(objs + [torch.zeros(1, self.W, device=dev)]).contiguous()
        self.d_off = torch.from_numpy(self.off.astype(np.int32)).to(dev)


def _raise_for_status(words, what):
    """the refusals of the reference, from the kernels' status words (host copies)"""
    st = int(np.bitwise_or.reduce(np.asarray(words, np.int64).reshape(-1), initial=0))
    if st & ST_OFFSETS:
        raise _lib.OdamError(f"{what}: target offsets or assignment indices outside their frame")
    if st & ST_CLASS:
        raise IndexError(f"{what}: a target label or angle bin is outside the classes of the output")
    if st & ST_DEGENERATE:
        raise AssertionError(f"{what}: a box with x1 < x0 or y1 < y0 (generalized_box_iou refuses degenerate boxes)")


class DegenerateBoxError(AssertionError, ValueError):
    """a degenerate box met while every decoder layer is scored: the reference's AssertionError (generalized_box_iou), which is
    also a ValueError about the batch handed in -- it names the layers and frames"""


def _raise_for_status_layers(words, what):
    """_raise_for_status for status words [L, B] of a layered call: the exception names every (layer, frame) that set the bit"""
    words = np.asarray(words, np.int64)
    st = int(np.bitwise_or.reduce(words.reshape(-1), initial=0))
    if not st:
        return
    L = words.shape[0]

    def where(bit):
        return "; ".join("layer %d%s: frame%s %s" % (l, " (last)" if l == L - 1 else "", "s" if np.count_nonzero(words[l] & bit) > 1 else "",
                                                      ", ".join(str(b) for b in np.nonzero(words[l] & bit)[0]))
                         for l in range(L) if (words[l] & bit).any())
    if st & ST_OFFSETS:
        raise _lib.OdamError(f"{what}: target offsets or assignment indices outside their frame ({where(ST_OFFSETS)})")
    if st & ST_CLASS:
        raise IndexError(f"{what}: a target label or angle bin is outside the classes of the output ({where(ST_CLASS)})")
    raise DegenerateBoxError(f"{what}: a box with x1 < x0 or y1 < y0 (generalized_box_iou refuses degenerate boxes) "
                             f"({where(ST_DEGENERATE)})")


def _layer_block(tensors):
    """[L] tensors of one shape (device, float32, contiguous) -> one [L, ...] tensor: the view over them when they already lie one
    after the other in one allocation (the blocks of Detector(..., aux=True)), else a stacked copy"""
    first, n = tensors[0], tensors[0].numel()
    if n and all(t.untyped_storage().data_ptr() == first.untyped_storage().data_ptr() and
                 t.data_ptr() == first.data_ptr() + 4 * n * l for l, t in enumerate(tensors)):
        return first.as_strided((len(tensors),) + tuple(first.shape), (n,) + tuple(first.stride()))
    return torch.stack(tensors).contiguous()


def match_cost_layers(S, logits, boxes, cost_class, cost_bbox, cost_giou):
    """odam_detr_match_cost_layers on logits / boxes [L, B, Q, .] and the staged targets S -> (cost float32 [L, Q * n_obj] -- one
    word per layer when no frame has a target -- and status int32 [L, B], both on the device)"""
    L = int(logits.shape[0])
    cost = torch.empty(L, max(S.Q * S.n_obj, 1), device=S.dev, dtype=torch.float32)
    status = torch.empty(L, max(S.B, 1), device=S.dev, dtype=torch.int32)
    with torch.cuda.device(S.dev):
        _lib.check(_entry("odam_detr_match_cost_layers")(
            _lib.ptr(logits), _lib.ptr(boxes), L, S.B, S.Q, S.n_logit, _lib.ptr(S.objects), _lib.ptr(S.d_off), S.n_obj, S.W,
            float(cost_class), float(cost_bbox), float(cost_giou), _lib.ptr(cost), _lib.ptr(status), _stream(S.dev)),
            "odam_detr_match_cost_layers")
    return cost, status[:, :S.B]


def match_cost(S, cost_class, cost_bbox, cost_giou):
    """odam_detr_match_cost on a staged batch -> (cost float32 [Q * n_obj] on the device, status int32 [B] on the device)"""
    cost = torch.empty(max(S.Q * S.n_obj, 1), device=S.dev, dtype=torch.float32)
    status = torch.empty(max(S.B, 1), device=S.dev, dtype=torch.int32)
    with torch.cuda.device(S.dev):
        _lib.check(_entry("odam_detr_match_cost")(
            _lib.ptr(S.t["pred_logits"]), _lib.ptr(S.t["pred_boxes"]), S.B, S.Q, S.n_logit, _lib.ptr(S.objects), _lib.ptr(S.d_off),
            S.n_obj, S.W, float(cost_class), float(cost_bbox), float(cost_giou), _lib.ptr(cost), _lib.ptr(status), _stream(S.dev)),
            "odam_detr_match_cost")
    return cost, status[:S.B]


def lsap_batch(cost, shapes, cost_off=None, device=None):
    """scipy.optimize.linear_sum_assignment of many cost blocks at once (odam_lsap_batch).  cost: float32 device tensor (any
    shape, read flat); shapes: [(rows, cols)] per problem; cost_off: element offset of every block (default: one after the other).
    Returns device tensors (col_of_row int32 [sum rows], n_pairs int32 [n], status int32 [n]) and the host's row offsets.
    Problems beyond 32 x 128 raise OdamError (ODAM_E_LIMIT) before anything is launched."""
    dev = cost.device if device is None else torch.device(device)
    shapes = [(int(r), int(c)) for r, c in shapes]
    n = len(shapes)
    if cost_off is None:
        cost_off = np.concatenate([[0], np.cumsum([r * c for r, c in shapes])])[:n]
    rows = np.asarray([r for r, _ in shapes], np.int32).reshape(n)
    cols = np.asarray([c for _, c in shapes], np.int32).reshape(n)
    m_off = np.concatenate([[0], np.cumsum(rows, dtype=np.int64)]).astype(np.int64)
    small = max([min(r, c) for r, c in shapes], default=0)
    large = max([max(r, c) for r, c in shapes], default=0)
    n_match = int(m_off[-1])
    col = torch.empty(max(n_match, 1), device=dev, dtype=torch.int32)
    info = torch.empty(2 * max(n, 1), device=dev, dtype=torch.int32)
    npairs, status = info[:n], info[max(n, 1):max(n, 1) + n]
    if n == 0:
        return col[:0], npairs, status, m_off
    d_off = torch.from_numpy(np.concatenate([np.asarray(cost_off, np.int64).reshape(n), m_off[:n]])).to(dev)      # cost_off | match_off
    d_shape = torch.from_numpy(np.concatenate([rows, cols])).to(dev)                                               # rows | cols
    cost = cost.contiguous()
    with torch.cuda.device(dev):
        _lib.check(_entry("odam_lsap_batch")(
            _lib.ptr(cost), int(cost.numel()), _lib.ptr(d_off), _lib.ptr(d_shape), ctypes.c_void_p(d_shape.data_ptr() + 4 * n), n,
            small, large, ctypes.c_void_p(d_off.data_ptr() + 8 * n), n_match, _lib.ptr(col), _lib.ptr(npairs), _lib.ptr(status),
            _stream(dev)), "odam_lsap_batch")
    col = col[:n_match]
    return col, npairs, status, m_off


def _lists(col_of_row):
    """scipy's (row_ind, col_ind) of one problem from its matched-column row (host array)"""
    i = np.nonzero(col_of_row >= 0)[0]
    return i.astype(np.int64), col_of_row[i].astype(np.int64)


def solve(cost, shapes, cost_off, dev):
    """the assignment of every block of a flat device cost buffer -> (col_of_row int32 [sum rows] on the device, the device
    solver's status words or None, the host's row offsets): odam_lsap_batch for the blocks inside 32 x 128, scipy itself on the
    host, from the block, for the others (where it raises ValueError as the reference's call does)"""
    shapes = [(int(r), int(c)) for r, c in shapes]
    cost_off = np.asarray(cost_off, np.int64).reshape(len(shapes))
    inside = [k for k, (r, c) in enumerate(shapes) if min(r, c) <= LSAP_MAX_SMALL and max(r, c) <= LSAP_MAX_LARGE]
    if len(inside) == len(shapes):
        col, _, status, m_off = lsap_batch(cost, shapes, cost_off, dev)
        return col, status, m_off
    from scipy.optimize import linear_sum_assignment
    m_off = np.concatenate([[0], np.cumsum([r for r, _ in shapes], dtype=np.int64)]).astype(np.int64)
    col = torch.full((int(m_off[-1]),), -1, device=dev, dtype=torch.int32)
    part, _, status, p_off = lsap_batch(cost, [shapes[k] for k in inside], cost_off[np.asarray(inside, np.int64)], dev)
    for n, k in enumerate(inside):
        col[m_off[k]:m_off[k + 1]] = part[p_off[n]:p_off[n + 1]]
    for k in sorted(set(range(len(shapes))) - set(inside)):
        r, c = shapes[k]
        i, j = linear_sum_assignment(cost.reshape(-1)[cost_off[k]:cost_off[k] + r * c].view(r, c).cpu().numpy())
        row = np.full(r, -1, np.int32)
        row[i] = j
        col[m_off[k]:m_off[k + 1]] = torch.from_numpy(row).to(dev)
    return col, (status if inside else None), m_off


def linear_sum_assignment_batch(cost_blocks):
    """[(row_ind, col_ind)] of a list of 2-D float32 cost blocks (device tensors or arrays), as scipy returns them (`solve` on
    the blocks laid one after the other).  Raises ValueError where scipy does."""
    blocks = [_f32(c, c.device if torch.is_tensor(c) and c.is_cuda else "cuda:0") for c in cost_blocks]
    if not blocks:
        return []
    dev = blocks[0].device
    flat = torch.cat([c.reshape(-1) for c in blocks] + [torch.zeros(1, device=dev)])
    shapes = [tuple(c.shape) for c in blocks]
    col, status, m_off = solve(flat, shapes, np.concatenate([[0], np.cumsum([r * c for r, c in shapes])])[:-1], dev)
    if status is not None and status.cpu().numpy().any():
        raise ValueError("linear_sum_assignment: cost matrix is infeasible or contains invalid numeric entries")
    col = col.cpu().numpy()
    return [_lists(col[m_off[k]:m_off[k + 1]]) for k in range(len(blocks))]


class HungarianMatcher:
    """matcher.py:11-82.  matcher(outputs, targets) -> [(index_i, index_j)] int64 CPU tensors per frame: the queries in ascending
    order and their targets, len = min(Q, G_b), as scipy.optimize.linear_sum_assignment lists them for the frame's cost block
        cost_bbox * L1(box) + cost_class * (-softmax[label]) + cost_giou * (-GIoU).
    (The reference's default cost_giou is 10; every caller of its build passes all three.)"""

    def __init__(self, cost_class=1, cost_bbox=1, cost_giou=1):
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"
        self.cost_class, self.cost_bbox, self.cost_giou = cost_class, cost_bbox, cost_giou

    def assign(self, S):
        """the assignment of a staged batch on the device -> (match int32 [B, Q]: target of every query or -1, [cost status [B],
        solver status] on the device).  Frames beyond the solver's 32 x 128 are solved by scipy from their cost block, which is
        the one copy to the host this makes."""
        cost, st_cost = match_cost(S, self.cost_class, self.cost_bbox, self.cost_giou)
        if any(min(S.Q, g) > LSAP_MAX_SMALL or max(S.Q, g) > LSAP_MAX_LARGE for g in S.sizes):
            _raise_for_status(st_cost.cpu().numpy(), "HungarianMatcher")      # before scipy reads a block that may hold no meaning
        col, st, _ = solve(cost, [(S.Q, g) for g in S.sizes], S.Q * S.off[:-1], S.dev)
        return col.view(S.B, S.Q), [st_cost] + ([st] if st is not None else [])

    def assign_layers(self, S, logits, boxes):
        """`assign` for logits / boxes [L, B, Q, .] of every decoder layer against the staged targets S: ONE cost launch and ONE
        solver launch over the L B problems -> (match int32 [L, B, Q], [cost status [L, B], solver status [L B]] on the device).
        The solver's limits and the host's scipy for a frame beyond them hold per problem, as in `assign`."""
        L = int(logits.shape[0])
        cost, st_cost = match_cost_layers(S, logits, boxes, self.cost_class, self.cost_bbox, self.cost_giou)
        if any(min(S.Q, g) > LSAP_MAX_SMALL or max(S.Q, g) > LSAP_MAX_LARGE for g in S.sizes):
            _raise_for_status_layers(st_cost.cpu().numpy(), "HungarianMatcher")      # before scipy reads a block that may hold no meaning
        per_layer = S.Q * S.n_obj
        off = np.concatenate([l * per_layer + S.Q * S.off[:-1] for l in range(L)])
        col, st, _ = solve(cost, [(S.Q, g) for g in S.sizes] * L, off, S.dev)
        return col.view(L, S.B, S.Q), [st_cost] + ([st] if st is not None else [])

    def __call__(self, outputs, targets):
        S = _Staged(outputs, targets, keys=("pred_logits", "pred_boxes"))
        match, words = self.assign(S)
        _raise_for_status(words[0].cpu().numpy(), "HungarianMatcher")
        if len(words) > 1 and words[1].cpu().numpy().any():
            raise ValueError("HungarianMatcher: cost matrix is infeasible or contains invalid numeric entries")
        m = match.cpu().numpy()
        return [tuple(torch.from_numpy(x) for x in _lists(m[b])) for b in range(S.B)]

    forward = __call__


class SetCriterion:
    """detr.py:258-481: criterion(outputs, targets) -> {key: 0-d float64 CPU tensor} under the reference's keys, for the requested
    `losses` (any of LOSS_NAMES; 'masks' is refused).  `matcher` is a HungarianMatcher of this module (the assignment then never
    leaves the device) or any callable returning the reference's list of (index_i, index_j).  When `outputs` holds a non-empty
    "aux_outputs" (Detector(..., aux=True), or the reference's list of dicts) every decoder layer is matched and scored as well, under
    "loss_*_{i}" and "cardinality_error_{i}" (no "class_error_{i}": the reference's log=False), with the call's num_boxes.
    After a call `last_partial` holds the per-frame partial sums [B, 11] (PARTIAL_KEYS) and `last_table` the whole table
    (TABLE_KEYS, with "total" over the weights of the requested losses) of the LAST layer, `last_partial_layers` [L, B, 11] and
    `last_table_layers` [L, 10] those of every layer in decoder order (L = 1 without aux_outputs), all on the device."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses):
        losses = list(losses)
        for name in losses:
            if name == "masks":
                raise _lib.OdamError("the segmentation losses (masks) are not part of this path")
            if name not in LOSS_NAMES:
                raise ValueError(f"do you really want to compute {name} loss? (one of {', '.join(LOSS_NAMES)})")
        self.num_classes, self.matcher, self.weight_dict, self.eos_coef, self.losses = num_classes, matcher, dict(weight_dict), eos_coef, losses
        self.last_partial = self.last_table = self.last_partial_layers = self.last_table_layers = None

    def _weights(self):
        want = {k for name in self.losses for k in KEYS_OF_LOSS[name]}
        return [float(self.weight_dict.get(k, 0.0)) if k in want else 0.0 for k in WEIGHT_KEYS]

    def total(self, losses):
        """sum(losses[k] * weight_dict[k]) over the keys both have, added in the order of WEIGHT_KEYS (the kernel's order); then
        the keys of the decoder layers 0, 1, ... ("loss_ce_0", ...), each layer in the order of WEIGHT_KEYS"""
        tot = 0.0
        for k in WEIGHT_KEYS:
            if k in losses and k in self.weight_dict and float(self.weight_dict[k]) != 0.0:
                tot = tot + float(self.weight_dict[k]) * losses[k]
        layers = sorted({int(k.rsplit("_", 1)[1]) for k in losses
                         if isinstance(k, str) and k.rsplit("_", 1)[-1].isdigit() and k.rsplit("_", 1)[0] in WEIGHT_KEYS})
        for i in layers:
            for base in WEIGHT_KEYS:
                k = f"{base}_{i}"
                if k in losses and k in self.weight_dict and float(self.weight_dict[k]) != 0.0:
                    tot = tot + float(self.weight_dict[k]) * losses[k]
        return torch.as_tensor(tot, dtype=torch.float64)

    def _call_layers(self, outputs, targets, num_boxes):
        """detr.py:441-481 with aux_outputs: the last layer and every entry of outputs["aux_outputs"], as ONE layered cost launch,
        ONE solver launch, the TWO layered criterion launches and one copy to the host.  The layers go to the kernels in decoder
        order (aux_outputs[0] first, the last layer in slot L-1); the "total" entry of every layer's table is formed with the
        weights of the unsuffixed keys."""
        last = {k: v for k, v in outputs.items() if k != "aux_outputs"}
        layers = list(outputs["aux_outputs"]) + [last]
        L = len(layers)
        S = _Staged(last, targets)
        if S.n_logit != self.num_classes + 1:
            raise ValueError(f"pred_logits have {S.n_logit} columns, the criterion was built for {self.num_classes} classes + no-object")
        if S.B < 1:
            raise ValueError("the criterion needs at least one frame")
        blk = {}
        for k in _OUT_KEYS:
            ts = []
            for i, d in enumerate(layers[:-1]):
                if k not in d:
                    raise KeyError(f"aux_outputs[{i}] has no {k!r}")
                if tuple(d[k].shape) != tuple(S.t[k].shape):
                    raise ValueError(f"aux_outputs[{i}][{k!r}] must be {list(S.t[k].shape)}, got {list(d[k].shape)}")
                ts.append(_f32(d[k], S.dev))
            blk[k] = _layer_block(ts + [S.t[k]])
        if isinstance(self.matcher, HungarianMatcher):
            match, words = self.matcher.assign_layers(S, blk["pred_logits"], blk["pred_boxes"])
        else:      # a caller's matcher: once per layer, as the reference calls it
            m = np.full((L, S.B, S.Q), -1, np.int32)
            for l, d in enumerate(layers):
                for b, (i, j) in enumerate(self.matcher(d, targets)):
                    m[l, b, np.asarray(i, np.int64)] = np.asarray(j, np.int64)
            match, words = torch.from_numpy(m).to(S.dev), []
        if num_boxes is None:
            num_boxes = max(S.n_obj, 1)
        n_ent, n_part = len(TABLE_KEYS), len(PARTIAL_KEYS)
        partial = torch.empty(L, S.B, n_part, device=S.dev, dtype=torch.float64)
        table = torch.empty(L, n_ent, device=S.dev, dtype=torch.float64)
        status = torch.empty(L, S.B, device=S.dev, dtype=torch.int32)
        w = (ctypes.c_double * len(WEIGHT_KEYS))(*self._weights())
        match = match.contiguous()
        with torch.cuda.device(S.dev):
            _lib.check(_entry("odam_detr_criterion_layers")(
                _lib.ptr(blk["pred_logits"]), _lib.ptr(blk["pred_boxes"]), _lib.ptr(blk["pred_angle"]), _lib.ptr(blk["pred_offset"]),
                _lib.ptr(blk["pred_size"]), _lib.ptr(blk["pred_depth"]), L, S.B, S.Q, S.n_logit, int(S.t["pred_angle"].shape[2]),
                _lib.ptr(S.objects), _lib.ptr(S.d_off), S.n_obj, S.W, _lib.ptr(match), float(num_boxes), float(self.eos_coef),
                ctypes.cast(w, ctypes.c_void_p), _lib.ptr(partial), _lib.ptr(table), _lib.ptr(status), _stream(S.dev)),
                "odam_detr_criterion_layers")
        # the one copy to the host: every layer's table and, behind them, the status words of the three calls
        tail = [x.reshape(-1).to(torch.float64) for x in words] + [status.reshape(-1).to(torch.float64)]
        host = torch.cat([table.reshape(-1)] + tail).cpu().numpy()
        lens = [len(x) for x in tail]
        st = np.split(host[L * n_ent:].astype(np.int64), np.cumsum(lens)[:-1])
        if words:
            _raise_for_status_layers(st[0].reshape(L, S.B), "SetCriterion (matcher)")
            if len(words) > 1 and st[1].any():
                raise ValueError("SetCriterion: cost matrix is infeasible or contains invalid numeric entries")
        _raise_for_status_layers(st[-1].reshape(L, S.B), "SetCriterion")
        self.last_partial_layers, self.last_table_layers = partial, table
        self.last_partial, self.last_table = partial[L - 1], table[L - 1]
        vals = host[:L * n_ent].reshape(L, n_ent)
        res = {k: torch.as_tensor(vals[L - 1][TABLE_KEYS.index(k)], dtype=torch.float64) for name in self.losses for k in KEYS_OF_LOSS[name]}
        for i in range(L - 1):      # the reference's log=False: no class_error of an aux layer
            res.update({f"{k}_{i}": torch.as_tensor(vals[i][TABLE_KEYS.index(k)], dtype=torch.float64)
                        for name in self.losses for k in KEYS_OF_LOSS[name] if k != "class_error"})
        return res

    def __call__(self, outputs, targets, num_boxes=None):
        if outputs.get("aux_outputs"):
            return self._call_layers(outputs, targets, num_boxes)
        S = _Staged(outputs, targets)
        if S.n_logit != self.num_classes + 1:
            raise ValueError(f"pred_logits have {S.n_logit} columns, the criterion was built for {self.num_classes} classes + no-object")
        if S.B < 1:
            raise ValueError("the criterion needs at least one frame")
        if isinstance(self.matcher, HungarianMatcher):
            match, words = self.matcher.assign(S)
        else:
            idx = self.matcher({k: v for k, v in outputs.items() if k != "aux_outputs"}, targets)
            m = np.full((S.B, S.Q), -1, np.int32)
            for b, (i, j) in enumerate(idx):
                m[b, np.asarray(i, np.int64)] = np.asarray(j, np.int64)
            match, words = torch.from_numpy(m).to(S.dev), []
        if num_boxes is None:
            num_boxes = max(S.n_obj, 1)
        n_ent, n_part = len(TABLE_KEYS), len(PARTIAL_KEYS)
        partial = torch.empty(S.B, n_part, device=S.dev, dtype=torch.float64)
        table = torch.empty(n_ent, device=S.dev, dtype=torch.float64)
        status = torch.empty(S.B, device=S.dev, dtype=torch.int32)
        w = (ctypes.c_double * len(WEIGHT_KEYS))(*self._weights())
        match = match.contiguous()
        with torch.cuda.device(S.dev):
            _lib.check(_entry("odam_detr_criterion")(
                _lib.ptr(S.t["pred_logits"]), _lib.ptr(S.t["pred_boxes"]), _lib.ptr(S.t["pred_angle"]), _lib.ptr(S.t["pred_offset"]),
                _lib.ptr(S.t["pred_size"]), _lib.ptr(S.t["pred_depth"]), S.B, S.Q, S.n_logit, int(S.t["pred_angle"].shape[2]),
                _lib.ptr(S.objects), _lib.ptr(S.d_off), S.n_obj, S.W, _lib.ptr(match), float(num_boxes), float(self.eos_coef),
                ctypes.cast(w, ctypes.c_void_p), _lib.ptr(partial), _lib.ptr(table), _lib.ptr(status), _stream(S.dev)),
                "odam_detr_criterion")
        # the one copy to the host: the table and, behind it, the status words of the three calls
        tail = [x.to(torch.float64) for x in words] + [status.to(torch.float64)]
        host = torch.cat([table] + tail).cpu().numpy()
        lens = [len(x) for x in tail]
        st = np.split(host[n_ent:].astype(np.int64), np.cumsum(lens)[:-1])
        if words:
            _raise_for_status(st[0], "SetCriterion (matcher)")
            if len(words) > 1 and st[1].any():
                raise ValueError("SetCriterion: cost matrix is infeasible or contains invalid numeric entries")
        _raise_for_status(st[-1], "SetCriterion")
        self.last_partial, self.last_table = partial, table
        self.last_partial_layers, self.last_table_layers = partial[None], table[None]
        vals = dict(zip(TABLE_KEYS, host[:n_ent]))
        return {k: torch.as_tensor(vals[k], dtype=torch.float64) for name in self.losses for k in KEYS_OF_LOSS[name]}

    forward = __call__


def build(args):
    """the criterion of detr.py:530-565 `build(args)` (its second return value) from the same keys: set_cost_class, set_cost_bbox,
    set_cost_giou (build_matcher), bbox_loss_coef, giou_loss_coef, eos_coef, dataset_file, and -- with a truthy aux_loss -- dec_layers:
    every weight again under "{key}_{i}" for the dec_layers - 1 aux layers (:556-560).  `args` is a namespace or a dict."""
    if isinstance(args, dict):
        g, has = args.__getitem__, args.__contains__
    else:
        g, has = (lambda k: getattr(args, k)), (lambda k: hasattr(args, k))
    ds = g("dataset_file") if has("dataset_file") else "scan_net"
    num_classes = 18 if ds == "scan_net" else (91 if ds == "coco" else 20)
    if has("masks") and g("masks"):
        raise _lib.OdamError("the segmentation losses (masks) are not part of this path")
    matcher = HungarianMatcher(cost_class=g("set_cost_class"), cost_bbox=g("set_cost_bbox"), cost_giou=g("set_cost_giou"))
    weight_dict = {"loss_ce": 1, "loss_bbox": g("bbox_loss_coef"), "loss_angle": 1, "loss_offset": 3, "loss_size": 1, "loss_depth": 1}
    weight_dict["loss_giou"] = g("giou_loss_coef")
    if has("aux_loss") and g("aux_loss"):
        aux_weight_dict = {}
        for i in range(g("dec_layers") - 1):
            aux_weight_dict.update({k + f"_{i}": v for k, v in weight_dict.items()})
        weight_dict.update(aux_weight_dict)
    return SetCriterion(num_classes, matcher=matcher, weight_dict=weight_dict, eos_coef=g("eos_coef"), losses=list(LOSS_NAMES))
