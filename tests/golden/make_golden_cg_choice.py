"""Records tests/golden/cg_choice.npz: which kernel launch_conv_gemm of a given checkout of this project (the parent of the commit
that introduced odam_amd/csrc/cg_choice.h) chooses for every row of tests/cg_choice_rows.py under every switch setting.

    python tests/golden/make_golden_cg_choice.py /path/to/checkout/of/the/parent

Needs hipcc and no GPU -- it must in fact run WITHOUT one: tests/native/cg_choice_record.hip calls the checkout's launch_conv_gemm with
placeholder operands and reads the noted token; the launch itself then fails.  The checkout's library is built with its own build
script if it is not there yet.

Arrays (integers only):
    rows [R, 41]       ConvGemmArgs: its integer fields, then its pointers as 0 / 1 (cg_choice_rows.FIELDS)
    settings [S, 13]   the switches (cg_choice_rows.SWITCHES)
    expect [R, S]      index into vocab: a token, "" for an empty problem (no launch), or "R <code> <odam_last_error>" for a refusal
    vocab              the distinct answers
    fields, switches   the column names;  parent: the commit recorded"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
import cg_choice_rows as T  # noqa: E402


def record(checkout, rows, settings, tmp):
    """the answers of the checkout's library, one string per (row, setting)"""
    lib = os.path.join(checkout, "odam_amd", "libodam_amd.so")
    if not os.path.exists(lib):
        subprocess.check_call([sys.executable, "-c", "import __graft_entry__ as g; g.build_library()"], cwd=checkout)
    exe = os.path.join(tmp, "cg_choice_record")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O1", "-std=c++17",
                           "-I", os.path.join(checkout, "odam_amd", "csrc"), os.path.join(REPO, "tests", "native", "cg_choice_record.hip"),
                           "-o", exe, "-L" + os.path.dirname(lib), "-lodam_amd", "-Wl,-rpath," + os.path.dirname(lib)])
    np.savetxt(os.path.join(tmp, "rows.txt"), rows, fmt="%d")
    np.savetxt(os.path.join(tmp, "settings.txt"), settings, fmt="%d")
    out = subprocess.run([exe, os.path.join(tmp, "rows.txt"), os.path.join(tmp, "settings.txt")], check=True, capture_output=True, text=True).stdout
    lines = out.split("\n")[:-1]
    assert len(lines) == len(rows) * len(settings), (len(lines), len(rows), len(settings))
    return ["" if ln == "N" else ln[2:] if ln[0] == "T" else ln for ln in lines]


def main(checkout):
    rows = np.asarray(T.all_rows(), np.int32)
    settings = np.asarray(T.all_settings(), np.int32)
    with tempfile.TemporaryDirectory() as tmp:
        answers = record(checkout, rows, settings, tmp)
    vocab = sorted(set(answers))
    index = {v: i for i, v in enumerate(vocab)}
    expect = np.asarray([index[a] for a in answers], np.int16).reshape(len(rows), len(settings))
    try:
        parent = subprocess.check_output(["git", "-C", checkout, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except subprocess.CalledProcessError:
        parent = os.environ["CG_CHOICE_PARENT"]      # an exported tree: name the commit
    path = os.path.join(HERE, "cg_choice.npz")
    np.savez_compressed(path, rows=rows, settings=settings, expect=expect, vocab=np.asarray(vocab), fields=np.asarray(T.FIELDS),
                        switches=np.asarray(T.SWITCHES), parent=np.asarray(parent))
    n_ref = sum(v.startswith("R ") for v in vocab)
    print("%s: %d rows x %d settings, %d answers (%d refusals), parent %s, %d bytes" %
          (path, len(rows), len(settings), len(vocab), n_ref, parent, os.path.getsize(path)))


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
