"""The table tests/test_cg_choice_host.py runs odam_cg::choose over (odam_amd/csrc/cg_choice.h): ConvGemmArgs as rows of integers and
the switch settings, built the way the library's callers build them -- detr_weights.hip pack_conv / pack_linear and the row-convolution
stem, detr_forward.hip conv_args / run_conv / stem_rows_t / fused_c2c3_t, assoc.hip lin, detr_ops.hip conv2d_op -- so that the rows are
the calls a forward makes.  tests/golden/make_golden_cg_choice.py records what the parent commit chose for every (row, setting)."""

# integer fields of ConvGemmArgs, then its pointers as null (0) / non-null (1); A, Wt and C are always non-null
INT_FIELDS = ["B", "H", "W", "Cin", "log2Cin", "Ho", "Wo", "Cout", "KH", "KW", "stride", "pad", "Kpad", "relu", "M", "ldc", "dtype", "out_f32",
              "lda", "k_order", "F_ldc", "F_relu", "G_N", "dil", "pool", "pool_ph", "pool_pw", "Hp", "Wp", "no_pin"]
PTR_FIELDS = ["Wt3", "scale", "bias", "res", "F_Wt3", "F_res", "F_C", "G_Wt3", "G_C", "F_Wt", "G_Wt"]
FIELDS = INT_FIELDS + PTR_FIELDS
ARG_DEFAULTS = dict({f: 0 for f in FIELDS}, G_N=64, dil=1)

# struct Switches, in its order, with the defaults of odam_common.hip
SWITCHES = ["ring", "f32", "fuse", "fuse_bf16", "s1", "ut", "tiles", "force", "presplit", "mfma16", "pin", "small_x3", "stem_pool"]
SWITCH_DEFAULTS = dict(ring=1, f32=2, fuse=2, fuse_bf16=2, s1=1, ut=1, tiles=31, force=0, presplit=1, mfma16=3, pin=0, small_x3=1, stem_pool=1)
LIM31 = 0x7fffffff
POOL_PH, POOL_PW = 8, 14
SIZES = [(2, 192, 256), (3, 601, 795), (32, 800, 1066), (42, 800, 1066)]
BLOCKS = {"r18": (True, [2, 2, 2, 2]), "r50": (False, [3, 4, 6, 3]), "r101": (False, [3, 4, 23, 3])}


def conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def split_planes_exist(dtype, Cout, Kpad):
    """detr_weights.hip upload_w3: a fp32 model keeps a layer's filters pre-split where they can be addressed"""
    return int(dtype == 0 and Kpad % 16 == 0 and Cout * Kpad * 6 < LIM31)


def pack_conv(dtype, Cin, Cout, KH, KW, stride, pad, dil=1):
    """detr_weights.hip pack_conv: the layer's integers"""
    epc = 8 if dtype else 4
    CinP = (Cin + epc - 1) // epc * epc
    kt, taps = 8 * epc, KH * KW
    Kpad = (taps * CinP + kt - 1) // kt * kt
    return dict(Cin=CinP, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad, dil=dil, Kpad=Kpad, k_order=int(1 < taps <= 32 and CinP % kt == 0),
                w3=split_planes_exist(dtype, Cout, Kpad))


def pack_linear(dtype, K, N):
    return dict(Cin=K, Cout=N, KH=1, KW=1, stride=1, pad=0, dil=1, Kpad=K, k_order=0, w3=split_planes_exist(dtype, N, K))


def conv_args(c, dtype, B, H, W):
    """detr_forward.hip conv_args"""
    a = dict(ARG_DEFAULTS)
    Ho = conv_out(H, (c["KH"] - 1) * c["dil"] + 1, c["stride"], c["pad"]); Wo = conv_out(W, (c["KW"] - 1) * c["dil"] + 1, c["stride"], c["pad"])
    a.update(dtype=dtype, Wt3=c["w3"], scale=1, bias=1, B=B, H=H, W=W, Cin=c["Cin"], log2Cin=(c["Cin"] - 1).bit_length(), Ho=Ho, Wo=Wo,
             Cout=c["Cout"], KH=c["KH"], KW=c["KW"], stride=c["stride"], pad=c["pad"], Kpad=c["Kpad"], dil=c["dil"], k_order=c["k_order"],
             M=B * Ho * Wo, ldc=c["Cout"])
    return a


def run_conv(c, dtype, B, H, W, res, relu, out_f32=0):
    """detr_forward.hip run_conv, with its power-of-two Cin / lda form of a one-tap layer of any width"""
    a = conv_args(c, dtype, B, H, W)
    a.update(out_f32=out_f32, res=int(res), relu=int(relu))
    if c["KH"] * c["KW"] == 1 and c["Cin"] & (c["Cin"] - 1):
        p2 = 1 << (c["Cin"] - 1).bit_length()
        a.update(Cin=p2, log2Cin=p2.bit_length() - 1, lda=c["Cin"])
    return a


def linear(dtype, K, N, M, res=False, relu=False, out_f32=0):
    return run_conv(pack_linear(dtype, K, N), dtype, 1, 1, M, res, relu, out_f32)


def stem_rows(dtype, B, ih, iw, pool):
    """detr_forward.hip stem_rows_t: conv1 as a 7x1 row convolution over the framed image, with or without the pool fields"""
    H1, W1 = conv_out(ih, 7, 2, 3), conv_out(iw, 7, 2, 3)
    Kp = 256 if dtype else 224
    c = dict(Cin=32, Cout=64, KH=7, KW=1, stride=2, pad=0, dil=1, Kpad=Kp, k_order=0 if dtype else 1, w3=split_planes_exist(dtype, 64, Kp))
    a = conv_args(c, dtype, B, ih + 6, iw + 8)
    a.update(lda=4, Ho=H1, Wo=W1, M=B * H1 * W1, relu=1)
    if pool:
        a.update(pool=1, pool_ph=POOL_PH, pool_pw=POOL_PW, Hp=conv_out(H1, 3, 2, 1), Wp=conv_out(W1, 3, 2, 1))
    return a


def fused(c2, c3, next_c1, dtype, B, H, W, res=True):
    """detr_forward.hip fused_c2c3_t: the 3x3 with the expand on its tile, and with the next block's reduce where next_c1 is given"""
    a = conv_args(c2, dtype, B, H, W)
    a.update(relu=1, F_res=int(res), F_C=1, F_ldc=c3["Cout"], F_relu=1)
    a["F_Wt" if dtype else "F_Wt3"] = 1
    if next_c1 is not None:
        a["G_Wt" if dtype else "G_Wt3"] = 1
        a.update(G_C=1, G_N=next_c1["Cout"])
    return a


def backbone_rows(name, dtype, B, ih, iw):
    """every contraction a forward of this backbone can issue, whichever way the switches send it: the layers one by one, and every
    fused form fused_c2c3_t offers to the predicates"""
    basic, blocks = BLOCKS[name]
    rows = [run_conv(pack_conv(dtype, 3, 64, 7, 7, 2, 3), dtype, B, ih, iw, False, True), stem_rows(dtype, B, ih, iw, True),
            stem_rows(dtype, B, ih, iw, False)]
    H, W = conv_out(conv_out(ih, 7, 2, 3), 3, 2, 1), conv_out(conv_out(iw, 7, 2, 3), 3, 2, 1)
    inpl = 64
    body = []
    for l, n in enumerate(blocks):
        for i in range(n):
            planes, stride = 64 << l, 2 if (i == 0 and l > 0) else 1
            if basic:
                b = dict(c1=pack_conv(dtype, inpl, planes, 3, 3, stride, 1), c2=pack_conv(dtype, planes, planes, 3, 3, 1, 1), stride=stride,
                         ds=pack_conv(dtype, inpl, planes, 1, 1, stride, 0) if (stride != 1 or inpl != planes) else None)
                inpl = planes
            else:
                b = dict(c1=pack_conv(dtype, inpl, planes, 1, 1, 1, 0), c2=pack_conv(dtype, planes, planes, 3, 3, stride, 1),
                         c3=pack_conv(dtype, planes, 4 * planes, 1, 1, 1, 0), stride=stride,
                         ds=pack_conv(dtype, inpl, 4 * planes, 1, 1, stride, 0) if i == 0 else None)
                inpl = 4 * planes
            body.append(b)
    for i, b in enumerate(body):
        Ho, Wo = conv_out(H, 3, b["stride"], 1), conv_out(W, 3, b["stride"], 1)
        rows.append(run_conv(b["c1"], dtype, B, H, W, False, True))
        if b["ds"]:
            rows.append(run_conv(b["ds"], dtype, B, H, W, False, False))
        if basic:
            rows.append(run_conv(b["c2"], dtype, B, Ho, Wo, True, True))
        else:
            rows.append(run_conv(b["c2"], dtype, B, H, W, False, True))
            rows.append(run_conv(b["c3"], dtype, B, Ho, Wo, True, True))
            rows.append(fused(b["c2"], b["c3"], None, dtype, B, H, W))
            nxt = body[i + 1]["c1"] if i + 1 < len(body) else None
            if nxt is not None and (dtype or (nxt["w3"] and nxt["Cout"] in (64, 128) and b["c3"]["Cout"] == 256)):      # fused_c2c3_t next_ok
                rows.append(fused(b["c2"], b["c3"], nxt, dtype, B, H, W))
        H, W = Ho, Wo
    rows.append(run_conv(pack_conv(dtype, inpl, 256, 1, 1, 1, 0), dtype, B, H, W, False, False))      # input_proj
    return rows, H * W


def transformer_rows(dtype, B, L, E, Q=100, ff=2048, dec_layers=6, n_cls=9):
    """encoder, stacked cross-attention keys / values, decoder and heads (detr_forward.hip): one row per distinct linear"""
    M, Mq = B * L, B * Q
    rows = []
    for m in (M, Mq):
        rows += [linear(dtype, E, 2 * E, m), linear(dtype, E, E, m), linear(dtype, E, E, m, res=True), linear(dtype, E, ff, m, relu=True),
                 linear(dtype, ff, E, m, res=True)]
    rows += [linear(dtype, E, dec_layers * E, M), linear(dtype, E, n_cls, Mq, out_f32=1), linear(dtype, E, E, Mq, relu=True)]
    rows += [linear(dtype, E, n, Mq, out_f32=1) for n in (4, 2, 1, 3)]
    return rows


def assoc_rows():
    """assoc.hip lin: the association network's linears (fp32, no_pin), at a few row counts"""
    rows = []
    for M in (37, 142, 4030):
        for K, N, lda, ldc, res, relu, scale in ((128, 256, 128, 256, 0, 1, 0), (256, 256, 256, 512, 1, 0, 0), (256, 768, 512, 768, 0, 0, 0),
                                                 (512, 768, 512, 768, 0, 0, 0), (256, 256, 256, 512, 0, 0, 0), (512, 512, 512, 512, 0, 1, 0),
                                                 (512, 256, 512, 512, 1, 0, 0), (256, 256, 512, 256, 0, 0, 0), (256, 30, 256, 32, 0, 0, 1)):
            a = dict(ARG_DEFAULTS)
            a.update(scale=scale, bias=1, res=res, B=1, H=1, W=M, Cin=K, lda=lda, log2Cin=(K - 1).bit_length(), Ho=1, Wo=M, Cout=N, KH=1, KW=1,
                     stride=1, pad=0, Kpad=K, relu=relu, M=M, ldc=ldc, no_pin=1)
            rows.append(a)
    return rows


def case_args(dtype, B, H, W, Cin, Cout, k, stride, pad, dil, relu, res, k_order, wt3, out_f32=0):
    """a row of CASES in tests/test_conv_f32_gpu.py / test_conv_bf16_gpu.py as detr_ops.hip conv2d_op hands it on; wt3: whether the
    entry split the filters for the call (presplit_applies under the case's switches)"""
    CinP = max(8, 1 << (Cin - 1).bit_length()) if dtype else (Cin + 3) // 4 * 4      # the modules' _pack
    kt = 64 if dtype else 32
    c = dict(Cin=CinP, Cout=Cout, KH=k, KW=k, stride=stride, pad=pad, dil=dil, Kpad=(k * k * CinP + kt - 1) // kt * kt, k_order=k_order, w3=0)
    c["w3"] = int(wt3 and split_planes_exist(dtype, Cout, c["Kpad"]))
    return run_conv(c, dtype, B, H, W, res, relu, out_f32)


def case_orders(dtype, Cin, k):
    return (0, 1) if Cin % (64 if dtype else 32) == 0 and k > 1 else (0,)


def refusal_and_limit_rows():
    """the shapes launch_conv_gemm refuses, the empty problems, and shapes one step below and one step above each 31-bit limit"""
    rows = []
    plain = lambda dtype, K, N, W, **kw: dict(linear(dtype, K, N, W), **kw)
    for dt in (0, 1):
        kt = 64 if dt else 32
        rows.append(dict(plain(dt, 64, 64, 4096), Cin=48, lda=0))                               # Cin not a power of two
        rows.append(plain(dt, 64, 64, 4096, Cin=2, log2Cin=1))                                  # less than one 16-byte chunk
        rows.append(plain(dt, 64, 64, 4096, Kpad=64 + kt // 2))                                 # Kpad off the k-tile
        rows.append(dict(conv_args(pack_conv(dt, 64, 64, 7, 7, 1, 3), dt, 2, 40, 40), k_order=1))     # 49 taps in k_order 1
        rows.append(dict(conv_args(pack_conv(dt, 64, 64, 8, 8, 1, 3), dt, 2, 40, 40)))          # KW 8
        rows.append(dict(conv_args(pack_conv(dt, 8, 64, 3, 3, 1, 1), dt, 2, 40, 40), k_order=1))      # k_order 1, Cin off the k-tile
        for nk in (2047, 2048):
            rows.append(plain(dt, kt, 64, 4096, Kpad=nk * kt, k_order=1))                       # k_order 1: k-tiles
        rows += [plain(dt, 64, 64, 4096, M=0), plain(dt, 64, 64, 4096, M=-5), plain(dt, 64, 64, 4096, Cout=0)]
        # asked for where it does not apply: the pool on a 256-channel layer, a fused call on a 256- / 512-channel 3x3 or a 1x1
        rows.append(dict(plain(dt, 64, 256, 200000), pool=1, pool_ph=POOL_PH, pool_pw=POOL_PW, Hp=1, Wp=100000, relu=1))
        for P in (32, 64, 128, 256, 512):
            for G in (0, 64, 128, 256):
                c2, c3 = pack_conv(dt, P, P, 3, 3, 1, 1), pack_conv(dt, P, 4 * P, 1, 1, 1, 0)
                for geom in ((32, 200, 267), (2, 48, 64)):
                    rows.append(fused(c2, c3, pack_conv(dt, 4 * P, G, 1, 1, 1, 0) if G else None, dt, *geom))
        a = fused(pack_conv(dt, 64, 64, 3, 3, 1, 1), pack_conv(dt, 64, 256, 1, 1, 1, 0), None, dt, 32, 200, 267)
        rows += [dict(a, dil=2), dict(a, F_C=0), dict(a, Wt3=0), dict(a, k_order=0), dict(a, KH=1, KW=1, Kpad=64, pad=0), dict(a, F_ldc=512)]
        # 31-bit limits.  Input span of a tile: 2 W lda esz + Cin esz bytes for one row of W > 256 pixels
        esz = 2 if dt else 4
        w_lim = (LIM31 - 64 * esz) // (2 * 64 * esz)
        for W in (w_lim, w_lim + 1):
            for Cout in (64, 128, 256):
                rows.append(plain(dt, 64, Cout, W))
        # filter bytes Cout Kpad esz, and the split planes' Cout Kpad 6 (few rows: the input span stays small)
        for Cout in (LIM31 // (65536 * esz), LIM31 // (65536 * esz) + 1):
            rows.append(plain(dt, 65536, Cout, 300))
        if not dt:
            for Cout in (LIM31 // (65536 * 6), LIM31 // (65536 * 6) + 1):
                rows.append(plain(0, 65536, Cout, 300, Wt3=1))
        # fused output bytes: one image Ho Wo F_ldc 4 (fp32), the whole tensor M F_ldc 2 (bf16)
        w_lim = (LIM31 // (256 * 4) if not dt else LIM31 // (256 * 2))
        for W in (w_lim, w_lim + 1):
            rows.append(fused(pack_conv(dt, 64, 64, 3, 3, 1, 1), pack_conv(dt, 64, 256, 1, 1, 1, 0), None, dt, 1, 1, W))
    return rows


def gpu_cases():
    """[(dtype, token, config, args)] of the CASES the two GPU modules assert on an MI355X"""
    import test_conv_bf16_gpu
    import test_conv_f32_gpu
    out = []
    for dtype, mod in ((0, test_conv_f32_gpu), (1, test_conv_bf16_gpu)):
        for tok, cfg, B, H, W, Cin, Cout, k, s, p, dil, relu, res, _ in mod.CASES:
            sw = dict(SWITCH_DEFAULTS, **{key.replace("cg_", "", 1): v for key, v in cfg.items()})
            wt3 = bool(sw["ring"]) and sw["f32"] == 2
            for k_order in case_orders(dtype, Cin, k):
                for out_f32 in ((0, 1) if dtype else (0,)):
                    out.append((dtype, tok, sw, case_args(dtype, B, H, W, Cin, Cout, k, s, p, dil, relu, res, k_order, wt3, out_f32)))
    return out


def all_rows(cases=True):
    """cases=False: without the rows of the GPU modules' CASES, which later changes may add to"""
    rows = []
    for B, ih, iw in SIZES:
        for dt in (0, 1):
            L = None
            for name in BLOCKS:
                r, L = backbone_rows(name, dt, B, ih, iw)
                rows += r
            for E in (256, 192, 320, 384):
                rows += transformer_rows(dt, B, L, E)
    rows += assoc_rows()
    for dtype, _, _, a in (gpu_cases() if cases else ()):
        rows += [dict(a, Wt3=0), dict(a, Wt3=split_planes_exist(dtype, a["Cout"], a["Kpad"]))]
    rows += refusal_and_limit_rows()
    seen, uniq = set(), []
    for a in rows:
        t = tuple(int(a[f]) for f in FIELDS)
        if t not in seen:
            seen.add(t); uniq.append(t)
    return uniq


def all_settings(cases=True):
    """the defaults, every key alone at each other documented value, and the combinations the GPU tests use"""
    out = [{}]
    single = dict(ring=(0, 2), f32=(0,), fuse=(0, 1), fuse_bf16=(0, 1), s1=(0,), ut=(0,), tiles=(0, 15, 23, 27, 29, 30), force=(1, 2, 3),
                  presplit=(0,), mfma16=(0, 1, 2), pin=(1,), small_x3=(0,), stem_pool=(0,))
    for k, vals in single.items():
        out += [{k: v} for v in vals]
    out += [dict(pin=1, mfma16=0), dict(pin=1, presplit=0), dict(pin=1, ring=2), dict(pin=1, ring=2, tiles=15), dict(pin=1, ring=2, tiles=23),
            dict(ring=2, mfma16=0), dict(ring=2, presplit=0), dict(pin=1, fuse=1), dict(pin=1, fuse=0), dict(pin=1, fuse_bf16=1),
            dict(pin=1, fuse_bf16=0), dict(pin=1, s1=0), dict(pin=1, ring=2, s1=0), dict(pin=1, stem_pool=0), dict(pin=1, f32=0), dict(pin=1, ring=0)]
    for _, _, sw, _ in (gpu_cases() if cases else ()):
        out.append({k: v for k, v in sw.items() if v != SWITCH_DEFAULTS[k]})
    uniq = []
    for s in out:
        t = tuple(dict(SWITCH_DEFAULTS, **s)[k] for k in SWITCHES)
        if t not in uniq:
            uniq.append(t)
    return uniq
