"""Which kernel a contraction runs on, without a GPU: odam_cg::choose (odam_amd/csrc/cg_choice.h) compiled by the host compiler
(tests/native/cg_choice_check.cpp) over tests/golden/cg_choice.npz -- every contraction of the R18 / R50 / R101 forwards and the
transformer at four batch sizes, the association network's, the cases of the two GPU conv modules, the refusals and the shapes on either
side of each 31-bit limit, under 47 switch settings -- against what launch_conv_gemm of the commit before cg_choice.h chose
(tests/golden/make_golden_cg_choice.py), and against the tokens an MI355X has asserted (CASES of test_conv_f32_gpu / test_conv_bf16_gpu)."""
import os
import subprocess

import numpy as np
import pytest

import cg_choice_rows as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_FIELDS = ["family", "code", "bm", "bn", "waves", "stages", "ut", "x3", "mode", "pool", "chain", "s1_window", "fused_second_ok",
              "fused_bf16_ok", "pooled_stem_ok"]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cg_choice") / "cg_choice_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", os.path.join(REPO, "tests", "native", "cg_choice_check.cpp"),
                           "-o", exe])
    return exe


def run_choose(exe, mode, rows, settings, tmp):
    """[{family, code, bm, ..., pooled_stem_ok, text}] per call; text = the token, or the message of a refusal"""
    np.savetxt(os.path.join(tmp, "rows.txt"), np.asarray(rows), fmt="%d")
    np.savetxt(os.path.join(tmp, "settings.txt"), np.asarray(settings), fmt="%d")
    p = subprocess.run([exe, mode, os.path.join(tmp, "rows.txt"), os.path.join(tmp, "settings.txt")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = []
    for ln in p.stdout.split("\n")[:-1]:
        head, text = ln.split(" | ", 1) if not ln.endswith(" | ") else (ln[:-3], "")
        v = head.split(" ")
        out.append(dict(zip(OUT_FIELDS, [v[0]] + [int(x) for x in v[1:]]), text=text))
    return out


@pytest.fixture(scope="module")
def table(check_exe, tmp_path_factory):
    """the fixture, and choose() on every (row, setting) of it: computed once, shared"""
    z = np.load(os.path.join(REPO, "tests", "golden", "cg_choice.npz"), allow_pickle=False)
    got = run_choose(check_exe, "cross", z["rows"], z["settings"], str(tmp_path_factory.mktemp("cg_table")))
    R, S = z["expect"].shape
    assert len(got) == R * S
    want = [str(z["vocab"][i]) for i in z["expect"].reshape(-1)]
    return z, got, want


def test_fixture_holds_the_rows_and_settings_asked_for(table):
    z = table[0]
    assert z["fields"].tolist() == T.FIELDS and z["switches"].tolist() == T.SWITCHES and len(str(z["parent"])) == 40
    # (the rows and settings of the GPU modules' CASES as they were when the fixture was recorded: cases added since are held to
    # their own token below, not to the parent's answer)
    assert set(T.all_rows(cases=False)) <= set(map(tuple, z["rows"].tolist()))
    assert set(T.all_settings(cases=False)) <= set(map(tuple, z["settings"].tolist()))
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "cg_choice.npz")) <= 256 * 1024
    rows = {f: z["rows"][:, i] for i, f in enumerate(T.FIELDS)}
    for B, ih, iw in T.SIZES:      # both stem forms at every size, in both types
        for dt in (0, 1):
            stem = (rows["B"] == B) & (rows["H"] == ih + 6) & (rows["W"] == iw + 8) & (rows["lda"] == 4) & (rows["dtype"] == dt)
            assert (stem & (rows["pool"] == 1)).sum() == 1 and (stem & (rows["pool"] == 0)).sum() == 1
    assert {192, 320, 384} <= set(rows["lda"].tolist()) and (rows["no_pin"] == 1).sum() >= 9
    for f in ("F_Wt3", "F_Wt", "G_Wt3", "G_Wt"):
        assert rows[f].sum() > 0
    answers = set(z["vocab"].tolist())
    assert "" in answers and sum(a.startswith("R 1 conv_gemm: ") for a in answers) == 5      # the five refusals of launch_conv_gemm


def test_choice_equals_the_parents(table):
    """every token, every refusal code and every message"""
    z, got, want = table
    S = len(z["settings"])
    bad = []
    for i, (g, w) in enumerate(zip(got, want)):
        if w == "":
            ok = g["family"] == "Nothing" and g["text"] == ""
        elif w.startswith("R "):
            code, msg = w[2:].split(" ", 1)
            ok = g["family"] == "Refused" and g["code"] == int(code) and g["text"] == msg
        else:
            ok = g["family"] not in ("Refused", "Nothing") and g["text"] == w
        if not ok:
            bad.append((dict(zip(T.FIELDS, z["rows"][i // S].tolist())), dict(zip(T.SWITCHES, z["settings"][i % S].tolist())), g, w))
    assert not bad, (len(bad), bad[:3])


def test_token_is_the_choice(table):
    """the fields of a Choice are what its token says (the launch switches on the fields)"""
    for g in table[1]:
        t = g["text"]
        if g["family"] == "Small":
            want = "%s.small.%dx%d.w%d%s%s%s" % (t.split(".")[0], g["bm"], g["bn"], g["waves"], ".ut" * g["ut"], ".x3" * g["x3"], ".s4" * (g["stages"] == 4))
            assert t == want and g["stages"] in (2, 4) and (g["bm"], g["bn"], g["waves"]) in ((128, 64, 8), (128, 64, 4), (64, 64, 4), (128, 128, 8), (128, 128, 4))
        elif g["family"] == "RingF32":
            assert t == "f32.ring.m%d.%dx%d%s" % (g["mode"], g["bm"], g["bn"], ".pool" * g["pool"]) and g["mode"] in (2, 3, 4)
            assert (g["bm"], g["waves"]) in ((256, 8), (512, 16)) and (g["waves"] == 8 or (g["mode"] == 4 and g["bn"] == 64))
        elif g["family"] == "RingBF16":
            assert t == "bf16.ring.%dx%d%s" % (g["bm"], g["bn"], ".pool" * g["pool"])
            assert (g["bm"], g["bn"], g["waves"]) in ((256, 256, 8), (256, 256, 16), (256, 128, 8), (256, 64, 8), (512, 64, 16))
        elif g["family"] == "FusedF32":
            kind = "l2" if g["bn"] == 128 else {0: "l1", 64: "chain64", 128: "chain128"}[g["chain"]]
            assert t == "f32.fused.m%d.%s" % (g["mode"], kind) and g["mode"] in (3, 4)
        elif g["family"] == "FusedBF16":
            assert t == "bf16.fused.p%d" % g["bn"] + (".chain%d" % g["chain"] if g["chain"] else "")
            assert (g["bn"], g["chain"]) in ((64, 0), (64, 64), (64, 128), (128, 0), (128, 128), (256, 0))


def test_s1_window_rules(table):
    """no token shows them: s1_window = cg.s1 for the 512-thread bf16 ring and the bf16 fused launches, 0 everywhere else"""
    z, got, _ = table
    S = len(z["settings"])
    s1 = z["settings"][:, T.SWITCHES.index("s1")]
    seen = set()
    for i, g in enumerate(got):
        windowed = (g["family"] == "RingBF16" and g["waves"] == 8) or g["family"] == "FusedBF16"
        assert g["s1_window"] == (int(s1[i % S]) if windowed else 0), (i, g)
        seen.add((g["family"], g["waves"], int(s1[i % S])))
    assert {("RingBF16", 8, 0), ("RingBF16", 8, 1), ("RingBF16", 16, 1), ("FusedBF16", 8, 0), ("FusedBF16", 8, 1), ("RingF32", 8, 1)} <= seen


def test_predicates_answer_as_the_launch(table):
    """fused_second_ok / fused_bf16_ok / pooled_stem_ok on the rows that ask: true exactly where the parent ran the fused / pooled kernel"""
    z, got, want = table
    S = len(z["settings"])
    col = {f: z["rows"][:, i] for i, f in enumerate(T.FIELDS)}
    n = {"f32.fused.": [0, 0], "bf16.fused.": [0, 0], ".pool": [0, 0]}
    for i, (g, w) in enumerate(zip(got, want)):
        r = i // S
        if col["M"][r] <= 0 or col["Cout"][r] <= 0 or w.startswith("R 1 conv_gemm: unsupported") or w.startswith("R 1 conv_gemm: k_order"):
            continue      # refused or empty before the question comes up
        if col["pool"][r]:
            assert g["pooled_stem_ok"] == int(w.endswith(".pool")), (i, g, w)
            n[".pool"][g["pooled_stem_ok"]] += 1
        elif col["F_Wt3"][r]:
            assert g["fused_second_ok"] == int(w.startswith("f32.fused.")), (i, g, w)
            n["f32.fused."][g["fused_second_ok"]] += 1
        elif col["F_Wt"][r]:
            assert g["fused_bf16_ok"] == int(w.startswith("bf16.fused.")), (i, g, w)
            n["bf16.fused."][g["fused_bf16_ok"]] += 1
    assert all(no > 100 and yes > 100 for no, yes in n.values()), n


def test_gpu_cases_get_the_token_they_assert(check_exe, table, tmp_path):
    """the rows of CASES in the two GPU conv modules, built as detr_ops.hip hands them on: the token an MI355X has asserted"""
    cases = T.gpu_cases()
    assert len(cases) > 100
    got = run_choose(check_exe, "zip", [[a[f] for f in T.FIELDS] for _, _, _, a in cases], [[sw[k] for k in T.SWITCHES] for _, _, sw, _ in cases],
                     str(tmp_path))
    for (dtype, tok, sw, a), g in zip(cases, got):
        assert g["text"] == tok, (tok, g, a, sw)
    # ... and the parent's recorded answer for the same row and setting is that token too
    z, _, want = table
    S = len(z["settings"])
    row_of = {tuple(r): i for i, r in enumerate(z["rows"].tolist())}
    set_of = {tuple(s): i for i, s in enumerate(z["settings"].tolist())}
    recorded = 0
    for dtype, tok, sw, a in cases:
        r, s = row_of.get(tuple(a[f] for f in T.FIELDS)), set_of.get(tuple(sw[k] for k in T.SWITCHES))
        if r is not None and s is not None:
            assert want[r * S + s] == tok
            recorded += 1
    assert recorded >= 100, recorded      # 147 when the fixture was recorded
