"""Host ingest on files that are wrong or merely odd (no GPU): the MatrixMarket loader, its binary cache, the run
file and the kernel JSON.  A file the loader cannot hold within its invariant (host/inc/sparse_matrix.h) is refused
with exit status 255 and one line that names what is wrong -- never an abort, a fault or a load; a legal file
loads bit for bit as the oracle's restatement of the reference's fscanf loop does.

The loader ends the process on a refusal and the oracle spins for ever on some inputs, so both run in child
processes (tests/host_ingest_child.py): one for all product loads, one, under a time limit, for all oracle loads."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, mtx
from host_ingest_child import damaged_caches

HOST = os.path.join(ROOT, "sparseharness_amd", "host")
KERNELS = os.path.join(HOST, "kernels")
CHILD = os.path.join(ROOT, "tests", "host_ingest_child.py")
COMBOS = [(e, n) for e in (0, 1) for n in (0, 1, 2)]          # element type x normaliser (none, PageRank, SCC)
THREADS = 4                                                   # OMP_NUM_THREADS of the product child: fixes the slices


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-s", "-C", HOST, "../libsparseharness_host.so", "bin/spmv_harness", "selftest"],
                          stderr=subprocess.DEVNULL)


def mm(banner, size, entries, comments="% made by the test\n", eol="\n", last_eol=True):
    return (f"%%MatrixMarket matrix coordinate {banner}{eol}{comments.replace(chr(10), eol)}{size}{eol}"
            + eol.join(entries) + (eol if last_eol else ""))


G, S = "real general", "real symmetric"
OK2 = ["1 2 2.0"]
# name -> (file text, what the one line on stderr must contain)
REFUSED = {
    "first_index_0": (mm(G, "3 3 2", OK2 + ["0 2 2.0"]), "first index (row) 0 outside 1..3"),
    "first_index_rows_plus_1": (mm(G, "3 3 2", OK2 + ["4 2 2.0"]), "first index (row) 4 outside 1..3"),
    "first_index_7": (mm(G, "3 3 2", OK2 + ["7 2 2.0"]), "first index (row) 7 outside 1..3"),
    "second_index_0": (mm(G, "3 3 2", OK2 + ["2 0 2.0"]), "second index (column) 0 outside 1..3"),
    "second_index_cols_plus_1": (mm(G, "3 3 2", OK2 + ["2 4 2.0"]), "second index (column) 4 outside 1..3"),
    "first_index_negative": (mm(G, "3 3 2", OK2 + ["-2147483648 2 2.0"]), "outside 1..3"),
    "sym_first_index_0": (mm(S, "3 3 2", OK2 + ["0 2 2.0"]), "outside 1..3"),
    "sym_first_index_rows_plus_1": (mm(S, "3 3 2", OK2 + ["4 2 2.0"]), "outside 1..3"),
    "sym_second_index_0": (mm(S, "3 3 2", OK2 + ["2 0 2.0"]), "outside 1..3"),
    "sym_second_index_cols_plus_1": (mm(S, "3 3 2", OK2 + ["2 4 2.0"]), "outside 1..3"),
    # legal as a general file; only its mirrored copy (4, 1) would lie outside: a symmetric file must be square
    "sym_mirrored_copy_outside": (mm(S, "3 4 1", ["1 4 1.0"]), "symmetric banner on a rectangular 3 x 4"),
    "rect_first_index_rows_plus_1": (mm(G, "2 5 2", ["1 4 1.0", "3 1 1.0"]), "first index (row) 3 outside 1..2"),
    "rect_second_index_cols_plus_1": (mm(G, "2 5 2", ["1 4 1.0", "1 6 1.0"]), "second index (column) 6 outside 1..5"),
    "tall_second_index_cols_plus_1": (mm(G, "5 2 2", ["4 1 1.0", "4 3 1.0"]), "second index (column) 3 outside 1..2"),
    "negative_rows": (mm(G, "-1 3 0", []), "negative number on the size line"),
    "negative_cols": (mm(G, "3 -1 0", []), "negative number on the size line"),
    "negative_rows_and_cols": (mm(G, "-1 -1 0", []), "negative number on the size line"),
    "negative_nnz": (mm(G, "3 3 -5", OK2), "negative number on the size line"),
    "nnz_doubled_overflows_int": (mm(S, "3 3 1073741825", OK2), "too many non-zeros"),
    "nnz_int_max": (mm(G, "3 3 2147483647", OK2), "ended early"),
    "nnz_int_max_pattern": (mm("pattern general", "3 3 2147483647", ["1 2"]), "ended early"),
    "fewer_entries_than_promised": (mm(G, "3 3 3", OK2 + ["2 3 1.0"]), "the file ended early"),
    "cut_after_first_index": (mm(G, "3 3 2", OK2 + ["2 "], last_eol=False), "ended early"),
    "cut_before_value": (mm(G, "3 3 2", OK2 + ["2 3"], last_eol=False), "ended early"),
    "cut_after_sign": (mm(G, "3 3 2", OK2 + ["2 3 -"], last_eol=False), "was not read as a number"),
    "cut_inside_exponent": (mm(G, "3 3 2", OK2 + ["2 3 1.5e"], last_eol=False), "was not read as a number"),
    "ends_after_banner": ("%%MatrixMarket matrix coordinate real general\n", "ended early, before the size line"),
    "ends_after_comments": ("%%MatrixMarket matrix coordinate real general\n% a\n% b\n", "ended early, before the size line"),
    "size_line_of_two": (mm(G, "3 3", []), "cannot read matrix sizes"),
    "empty_file": ("", "Could not read matrix market banner"),
    "value_is_no_number": (mm(G, "3 3 2", ["1 2 abc", "2 3 1.0"]), 'token "abc" was not read as a number'),
    "index_is_no_number": (mm(G, "3 3 2", ["1 x 1.0", "2 3 1.0"]), 'token "x" was not read as a number'),
    "index_is_a_fraction": (mm(G, "3 3 2", ["1.5 2 1.0", "2 3 1.0"]), "was not read as a number"),
    "value_runs_into_text": (mm(G, "3 3 2", ["1 2 1.0abc", "2 3 1.0"]), "was not read as a number"),
    # the reference's fscanf loop stalls on the '%' and files every later entry under row -1: refused here
    "comment_between_entries": (mm(G, "3 3 2", ["1 2 1.0", "% a comment", "2 3 1.0"]), 'token "%" was not read as a number'),
}

E4 = ["1 2 2.5", "3 1 -7.75", "4 3 16", "2 4 3", "2 2 -1.25"]
# name -> file text; legal, if odd: the oracle decides what the rows are
ODD = {
    "plain": mm(G, "4 4 5", E4),
    "crlf_line_ends": mm(G, "4 4 5", E4, eol="\r\n"),
    "blank_line_before_size_line": mm(G, "4 4 5", E4, comments="% c\n\n"),
    "mixed_case_banner": "%%MatrixMarket MATRIX Coordinate REAL General\n4 4 5\n" + "\n".join(E4) + "\n",
    "upper_case_banner": "%%MatrixMarket MATRIX COORDINATE INTEGER SYMMETRIC\n4 4 2\n2 1 5\n4 4 -3\n",
    "no_final_newline": mm(G, "4 4 5", E4, last_eol=False),
    "more_entries_than_promised": mm(G, "4 4 2", E4),
    "more_entries_than_promised_symmetric": mm(S, "4 4 1", ["2 1 2.5", "3 1 1.5"]),
    "hermitian_banner": mm("real hermitian", "4 4 3", ["2 1 2.5", "3 1 -7.75", "4 4 2"]),
    "skew_symmetric_banner": mm("real skew-symmetric", "4 4 2", ["2 1 2.5", "3 1 -7.75"]),
    "plus_sign_on_an_index": mm(G, "4 4 2", ["+1 +2 +2.5", "3 +1 -7.75"]),
    "duplicates_in_a_symmetric_file": mm(S, "4 4 5", ["2 1 2.5", "2 1 2.5", "3 1 4", "1 3 4", "4 4 9"]),
    "explicit_zeros": mm(G, "4 4 4", ["1 2 0", "3 1 0.0", "4 3 -0.0", "2 4 3"]),
    "pattern_general": mm("pattern general", "4 4 3", ["1 2", "3 1", "4 4"]),
    "pattern_symmetric": mm("pattern symmetric", "4 4 3", ["2 1", "3 1", "4 4"]),
    "integer_general": mm("integer general", "4 4 3", ["1 2 -5", "3 1 7", "4 3 0"]),
    "blanks_and_tabs": mm(G, "4 4 3", ["  1   2\t2.5  ", "\t3 1 -7.75", "4\t\t3    16\t"]),
    "entries_across_lines": mm(G, "4 4 3", ["1", "2 2.5 3", "1 -7.75", "4 3", "16"]),
    "comments_before_size_line": mm(G, "4 4 5", E4, comments="%\n%%%\n% 9 9 9\n"),
    "no_rows_at_all": mm(G, "0 0 0", []),
    "no_entries": mm(G, "4 4 0", []),
}

# Two inputs on which the oracle, like the reference's mmio, spins for ever: never given to it.  The product
# skips both comments: a comment is a line whose first non-blank character is '%', of any length.
E3 = ["1 2 5.0", "3 1 7.0"]
WRITTEN_OUT = {   # name -> (text, rows, cols, row_ptr, col_idx, values): row = file column, column = file row
    "comment_longer_than_1024": (mm(G, "3 3 2", E3, comments="% " + "x" * 3000 + "\n"), 3, 3, [0, 1, 2, 2], [2, 0], [7, 5]),
    "indented_comment": (mm(G, "3 3 2", E3, comments="   % 1 2 3\n\t%\n"), 3, 3, [0, 1, 2, 2], [2, 0], [7, 5]),
    # Rectangular files are loaded, with as many rows as the file has columns (the reference sizes the rows by the
    # file's row count and overruns them): more columns than rows, then more rows than columns
    "wide_2_by_5": (mm(G, "2 5 2", ["1 4 3.0", "2 5 4.0"]), 5, 2, [0, 0, 0, 0, 1, 2], [0, 1], [3, 4]),
    "tall_4_by_2": (mm(G, "4 2 3", ["4 1 3.0", "1 2 4.0", "3 2 5.0"]), 2, 4, [0, 1, 3], [3, 0, 2], [3, 4, 5]),
}

# `int` conversion of these is undefined, in the oracle too: untruncated float loads only, against numpy
SPECIAL = ["inf", "-inf", "nan", "Infinity", "1e40", "-1e39", "0x1.8p1", "0X1P-3", "-0x1.fffffep127", "2147483648",
           "-2147483649.5", "4294967296", "1e10", "3.4028235e38", "3.4028236e38", "1e-46"]


def special_value(text):
    with np.errstate(over="ignore", under="ignore"):
        return np.float32(np.float64(float.fromhex(text) if "x" in text.lower() else text))


# ---- files of the sliced (OpenMP) tokenizer's size: >= 50 000 entries, body > 1 MiB
BIG_N, BIG_M = 60_000, 120_000


def big_entries():
    """Entries of very different line lengths (6 to ~70 bytes) in random order, so that whatever lies around a
    slice's cut point -- body * t / nthreads, moved to the next line end -- is a mix of short and long lines."""
    rng = np.random.default_rng(11)
    I, J = rng.integers(1, BIG_N + 1, BIG_M), rng.integers(1, BIG_N + 1, BIG_M)
    V, kind = rng.uniform(-1e4, 1e4, BIG_M), rng.integers(0, 3, BIG_M)
    out = []
    for a, b, v, k in zip(I.tolist(), J.tolist(), V.tolist(), kind.tolist()):
        out.append(f"{a} {b} {int(v) % 10}" if k == 0 else f"{a}  {b}\t{v:.9f} " if k == 1 else
                   f"   {a}          {b}     {v:.15e}" + " " * 24)
    return out


def big_text(entries, promised=BIG_M):
    return f"%%MatrixMarket matrix coordinate real general\n% big\n{BIG_N} {BIG_N} {promised}\n" + "\n".join(entries) + "\n"


def slice_cut_lines(text, t):
    """(last entry of slice t - 1, first entry of slice t), as indices into the entries, for THREADS slices: the
    loader cuts at body * t / nthreads and moves on to the next line end."""
    start = text.index("\n", text.index("\n", text.index("\n") + 1) + 1) + 1   # behind banner, comment, size line
    body = len(text) - start
    assert body > (1 << 20) and THREADS <= body // (256 << 10) + 1
    q = text.index("\n", start + body * t // THREADS)
    last = text.count("\n", start, q)           # the line the cut point lies in
    return last, last + 1


BAD_INDEX = {"first_0": lambda a, b, v: f"0 {b} {v}", "first_rows_plus_1": lambda a, b, v: f"{BIG_N + 1} {b} {v}",
             "second_0": lambda a, b, v: f"{a} 0 {v}", "second_cols_plus_1": lambda a, b, v: f"{a} {BIG_N + 1} {v}"}


PLACES = ["first_slice", "last_slice", "last_entry", "end_of_a_slice", "start_of_a_slice", "start_of_last_slice"]
BIG_NAMES = (["big_clean", "big_three_entries_short", "big_cut_mid_token", "big_value_is_no_number"]
             + [f"big_{kind}_at_{place}" for kind in BAD_INDEX for place in PLACES])


def big_files():
    """name -> (text, needle on stderr, parse path the loader must report)."""
    base = big_entries()
    clean = big_text(base)
    end_of_first, start_of_second = slice_cut_lines(clean, 1)
    end_of_third, start_of_last = slice_cut_lines(clean, THREADS - 1)
    assert 100 < end_of_first < start_of_last < BIG_M - 100
    places = {"first_slice": 7, "last_slice": BIG_M - 2, "last_entry": BIG_M - 1, "end_of_a_slice": end_of_first,
              "start_of_a_slice": start_of_second, "start_of_last_slice": start_of_last}
    files = {"big_clean": (clean, None, "ok")}
    for kind, bad in BAD_INDEX.items():
        for place, k in places.items():
            e = list(base)
            e[k] = bad(*base[k].split())
            text = big_text(e)
            if "slice" in place and place not in ("first_slice", "last_slice"):   # the swap moved no cut past the entry
                t = 1 if place != "start_of_last_slice" else THREADS - 1
                assert k in slice_cut_lines(text, t), (kind, place)
            files[f"big_{kind}_at_{place}"] = (text, "outside 1..%d" % BIG_N, "ok")
    files["big_three_entries_short"] = (big_text(base[:-3]), "ended early: entry %d of %d" % (BIG_M - 2, BIG_M), "fell back")
    files["big_cut_mid_token"] = (big_text(base[:-1] + ["17 23 -"]).rstrip("\n"), "was not read as a number", "fell back")
    files["big_value_is_no_number"] = (big_text(base[:start_of_second] + ["17 23 abc"] + base[start_of_second + 1:]),
                                       'token "abc" was not read as a number', "fell back")
    assert sorted(files) == sorted(BIG_NAMES) and list(places) == PLACES
    return files


def key(name, e, n):
    return f"{name}.e{e}.n{n}"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Every file of this module on disk once: name -> path, and what the big ones expect."""
    d = tmp_path_factory.mktemp("ingest")
    paths, big = {}, big_files()
    texts = {**{k: v[0] for k, v in REFUSED.items()}, **ODD, **{k: v[0] for k, v in WRITTEN_OUT.items()},
             **{k: v[0] for k, v in big.items()}}
    n = len(SPECIAL)
    texts["special_values"] = mm(G, f"{n} {n} {n}", [f"{i + 1} {(i * 5) % n + 1} {v}" for i, v in enumerate(SPECIAL)])
    for name, text in texts.items():
        paths[name] = str(d / (name + ".mtx"))
        with open(paths[name], "w", newline="") as f:
            f.write(text)
    return {"dir": d, "paths": paths, "big": {k: v[1:] for k, v in big.items()}}


class Loads:
    def __init__(self, outdir, status):
        self.outdir, self.status = outdir, status

    def stderr(self, k):
        with open(os.path.join(self.outdir, k + ".err"), errors="replace") as f:
            return f.read()

    def arrays(self, k):
        z = np.load(os.path.join(self.outdir, k + ".npz"))
        return z["dims"].tolist(), z["row_ptr"], z["col_idx"], z["val"]


@pytest.fixture(scope="module")
def product(files):
    """Every product load of this module, each in a child process of its own (one fork per load)."""
    out = files["dir"] / "product"
    out.mkdir()
    jobs = []
    for name, path in files["paths"].items():
        for e, n in COMBOS:
            jobs.append({"key": key(name, e, n), "path": path, "elem_is_int": e, "normalise": n, "truncate": 1,
                         "env": {"SH_LOG_LEVEL": "4"} if name.startswith("big_") else {}})
    jobs.append({"key": "special_values.raw", "path": files["paths"]["special_values"], "elem_is_int": 0, "normalise": 0,
                 "truncate": 0, "env": {}})
    jobs = [j for j in jobs if not (j["key"].startswith("special_values.e"))]
    (out / "jobs.json").write_text(json.dumps(jobs))
    env = {k: v for k, v in os.environ.items() if k not in ("SH_CSR_CACHE", "SH_NO_TRUNCATE", "SH_LOG_LEVEL")}
    r = subprocess.run([sys.executable, CHILD, "product", str(out), str(out / "jobs.json")], capture_output=True, text=True,
                       env=dict(env, OMP_NUM_THREADS=str(THREADS)), timeout=600)
    assert r.returncode == 0, r.stderr[-800:]
    return Loads(str(out), json.loads((out / "status.json").read_text()))


@pytest.fixture(scope="module")
def oracle(files):
    """The oracle's rows of every legal file, from one child process under a time limit."""
    out = files["dir"] / "oracle"
    out.mkdir()
    names = list(ODD) + ["big_clean"]
    jobs = [{"key": key(name, e, 0), "path": files["paths"][name], "elem_is_int": e, "normalise": 0} for name in names
            for e in (0, 1)]
    (out / "jobs.json").write_text(json.dumps(jobs))
    try:
        r = subprocess.run([sys.executable, CHILD, "oracle", str(out), str(out / "jobs.json")], capture_output=True, text=True,
                           timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("the oracle did not return on " + (out / "progress").read_text())
    assert r.returncode == 0, r.stderr[-800:]
    return Loads(str(out), {})


def assert_invariant(dims, rp, ci, va):
    rows, cols, _ = dims
    assert len(rp) == rows + 1 and rp[0] == 0 and rp[-1] == len(ci) == len(va) and (np.diff(rp) >= 0).all()
    assert ((ci >= 0) & (ci < cols)).all()


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_malformed_file_is_refused(product, name):
    for e, n in COMBOS:
        k = key(name, e, n)
        err = product.stderr(k)
        assert product.status[k] == 255, (k, product.status[k], err[-300:])      # exit(-1): no abort, fault or load
        said = [l for l in err.splitlines() if REFUSED[name][1] in l]
        assert len(said) == 1, (k, err[-300:])
        assert "Bad matrix file" in said[0] or name == "empty_file"
        if "no_number" in name or "cut_" in name or "fewer" in name or "comment" in name:
            assert "outside" not in err                                          # not "index 0 outside": the token is named


@pytest.mark.parametrize("name", sorted(ODD))
def test_odd_but_legal_file_loads_as_the_oracle_does(product, oracle, name):
    for e in (0, 1):
        k = key(name, e, 0)
        assert product.status[k] == 0, (k, product.stderr(k)[-300:])
        got, want = product.arrays(k), oracle.arrays(k)
        assert got[0] == want[0]
        for a, b in zip(got[1:], want[1:]):
            np.testing.assert_array_equal(a, b)                                  # values as uint32: bit for bit
    for e, n in COMBOS:                                                          # and under the normalisers it loads soundly
        assert product.status[key(name, e, n)] == 0
        assert_invariant(*product.arrays(key(name, e, n)))


@pytest.mark.parametrize("name", sorted(WRITTEN_OUT))
def test_comments_and_rectangular_files_load_as_written_out(product, name):
    _, rows, cols, rp, ci, va = WRITTEN_OUT[name]
    for e, n in COMBOS:
        k = key(name, e, n)
        assert product.status[k] == 0, (k, product.stderr(k)[-300:])
        dims, grp, gci, gva = product.arrays(k)
        assert dims == [rows, cols, len(ci)]
        np.testing.assert_array_equal(grp, rp)
        np.testing.assert_array_equal(gci, ci)
        assert_invariant(dims, grp, gci, gva)
        if n == 0:
            np.testing.assert_array_equal(gva.view(np.int32 if e else np.float32), va)


def test_rectangular_file_still_ends_the_app_as_not_square(files):
    for name in ("wide_2_by_5", "tall_4_by_2"):
        r = subprocess.run([os.path.join(HOST, "bin", "spmv_harness"), "-m", files["paths"][name], "-f", "m", "-k",
                            os.path.join(KERNELS, "spmv.json"), "-r", os.path.join(KERNELS, "runfile.csv"), "-n", "h", "-e", "e",
                            "--gold_only"], capture_output=True, text=True)
        assert r.returncode == 2 and "Matrix is not square" in r.stdout


def test_special_values_untruncated(product):
    assert product.status["special_values.raw"] == 0, product.stderr("special_values.raw")[-300:]
    dims, rp, ci, va = product.arrays("special_values.raw")
    n = len(SPECIAL)
    assert dims == [n, n, n]
    want = {((i * 5) % n, i): special_value(v) for i, v in enumerate(SPECIAL)}      # (row, column) -> value
    for r in range(n):
        for j in range(rp[r], rp[r + 1]):
            assert va[j] == want[(r, ci[j])].view(np.uint32), SPECIAL[ci[j]]


@pytest.mark.parametrize("name", sorted(BIG_NAMES))
def test_both_parse_paths_refuse_alike(files, product, oracle, name):
    """The sliced tokenizer sees these files first (the loader logs which path gave the entries): a bad entry in the
    first slice, in the last, or on either side of a cut is refused as it is in a small file."""
    needle, path = files["big"][name]
    for e, n in COMBOS:
        k = key(name, e, n)
        err = product.stderr(k)
        assert f"parallel MatrixMarket parse on {THREADS} threads: {path}" in err, err[-300:]
        if needle is None:
            assert product.status[k] == 0
            continue
        assert product.status[k] == 255, (k, product.status[k], err[-300:])
        assert len([l for l in err.splitlines() if needle in l and "Bad matrix file" in l]) == 1, err[-300:]
    if needle is None:                       # the clean file: what the slices give is what the oracle gives
        for e in (0, 1):
            got, want = product.arrays(key(name, e, 0)), oracle.arrays(key(name, e, 0))
            assert got[0] == want[0]
            for a, b in zip(got[1:], want[1:]):
                np.testing.assert_array_equal(a, b)


# ---- run file and kernel JSON ------------------------------------------------------------------------------------

def gold_only(*extra, runfile=None, kernel=None):
    return subprocess.run([os.path.join(HOST, "bin", "spmv_harness"), "-m", mtx("matrix3"), "-f", "m", "-k",
                           kernel or os.path.join(KERNELS, "spmv.json"), "-r", runfile or os.path.join(KERNELS, "runfile.csv"),
                           "-n", "h", "-e", "e", "--gold_only", *extra], capture_output=True, text=True)


@pytest.mark.parametrize("line", ["1280,1,1,256,1", "1280,1,1", "1280,1,1,256,1,1,1", "1280,1,x,256,1,1", "1280,1,,256,1,1",
                                  "1280,1,-1,256,1,1", "1280;1;1;256;1;1"])
def test_bad_run_file_line_ends_the_app_with_a_message(tmp_path, line):
    rf = tmp_path / "runs.csv"
    rf.write_text("1280,1,1,256,1,1\n" + line + "\n")
    r = gold_only(runfile=str(rf))
    assert r.returncode == 255 and "Bad run file line" in r.stderr, (r.returncode, r.stderr[-300:])
    assert gold_only().returncode == 0


def test_bad_kernel_file_ends_the_app_with_a_message(tmp_path):
    good = open(os.path.join(KERNELS, "spmv.json")).read()
    cases = {"cut": good[:len(good) // 2], "deep": "[" * 100_000, "escape": good.replace("csr-stream", "csr\\u12zzstream"),
             "string": good.replace('"csr-stream"', '"csr-stream'), "properties": good.replace('"properties"', '"propertys"'),
             "chunk": good.replace('"outerMap"', '"chunkSize": "abc", "outerMap"')}
    for name, text in cases.items():
        assert text != good
        k = tmp_path / (name + ".json")
        k.write_text(text)
        r = gold_only(kernel=str(k))
        assert r.returncode == 255 and "Bad kernel file" in r.stderr, (name, r.returncode, r.stderr[-300:])


def test_selftest_refuses_every_prefix_of_a_shipped_kernel_file(tmp_path):
    r = subprocess.run([os.path.join(HOST, "bin", "host_selftest"), str(tmp_path), os.path.join(KERNELS, "spmv.json")],
                       capture_output=True, text=True, env={**os.environ, "SH_QUIET_TIMERS": "1"})
    assert r.returncode == 0 and "all passed" in r.stdout, r.stdout[-800:]
    m = re.search(r"kernel file prefixes refused: (\d+) of (\d+)", r.stdout)
    assert m and m.group(1) == m.group(2) and int(m.group(2)) > 900


class Num(float):
    """Python's arithmetic with the evaluator's one rule of its own: x / 0 is 0."""
    def __add__(s, o): return Num(float(s) + float(o))
    def __sub__(s, o): return Num(float(s) - float(o))
    def __mul__(s, o): return Num(float(s) * float(o))
    def __truediv__(s, o): return Num(float(s) / float(o) if float(o) != 0 else 0.0)
    def __neg__(s): return Num(-float(s))
    def __pos__(s): raise SyntaxError("no unary plus in a size expression")


SIZES = {"v_MWidthC_1": 18, "v_MHeight_2": 1138, "v_VLength_3": 1200}
EXPRESSIONS = [
    "4", "(4)", "((4))", "4*v_MHeight_2", "(4*v_MHeight_2*v_MWidthC_1)", "(4*v_VLength_3)", "2+3*4", "(2+3)*4", "2*3+4", "2*(3+4)",
    "20-3-4", "20-(3-4)", "100/5/2", "100/(5/2)", "7/2", "7/2*2", "-7/2", "1-7/2", "-3", "--3", "-(2+3)", "2*-3", "2--3", "-v_MWidthC_1*2",
    "(8+(4*v_MWidthC_1))/2", "((v_MHeight_2+127)/128)*128", "v_MHeight_2/0", "5+4/0", "4/(2-2)*3+1", "0/0", " 4 * v_MHeight_2 ",
    "\t( 2 +\t3 ) * 4", "4 *", "* 4", "4 4", "4+", "(4", "4)", "((4)", "()", "", " ", "?", "v_Unknown", "(4*v_Unknown)", "v_MHeight_2x",
    "v_mheight_2", "4*v_MHeight_2 trailing", "4;5", "4,5", "1.5", "1e3", "0x10", "2**3", "7%2", "+3", "2++3", "4*(v_MHeight_2+(v_MWidthC_1*(2+v_VLength_3)))",
    "2147483647", "2147483647+1", "-2147483648", "-2147483649", "65536*65536", "4*v_MHeight_2*v_MHeight_2*v_MHeight_2", "1/3*3", "2/3+2/3",
]


def python_value(expr):
    """Python's own evaluation of the text, every literal and name a Num; what Python refuses, and what does not fit
    an int, is 0."""
    try:
        v = eval(re.sub(r"(?<![\w.])(\d+)(?![\w.])", r"Num(\1)", expr), {"__builtins__": {}, "Num": Num},
                 {k: Num(x) for k, x in SIZES.items()})
        return int(v) if isinstance(v, Num) and -2 ** 31 <= int(v) < 2 ** 31 else 0
    except Exception:
        return 0


def evaluate(exprs, w, h, v):
    r = subprocess.run([os.path.join(HOST, "bin", "host_selftest"), "--eval", str(w), str(h), str(v), *exprs], capture_output=True,
                       text=True)
    assert r.returncode == 0
    return [int(l) for l in r.stdout.split()]


def test_size_expressions_against_python():
    assert len(EXPRESSIONS) >= 30
    got = evaluate(EXPRESSIONS, SIZES["v_MWidthC_1"], SIZES["v_MHeight_2"], SIZES["v_VLength_3"])
    want = [python_value(e) for e in EXPRESSIONS]
    assert got == want, [(e, g, w) for e, g, w in zip(EXPRESSIONS, got, want) if g != w]
    assert sum(w != 0 for w in want) >= 30                    # the table is not all refusals


def test_size_expressions_of_every_kernel_file_at_the_headline_sizes():
    """Height 10 000 000 with MWidthC the widest row of the power-law workload (2 400 000 entries, the row the
    headline test's docstring speaks of; ragged kernels get the matrix width): a size that does not fit an int
    evaluates to 0, as an unparseable one does, and every other one to its value."""
    import glob
    h, widest = 10_000_000, 2_400_000
    files = sorted(glob.glob(os.path.join(KERNELS, "*.json")) + glob.glob(os.path.join(GOLDEN, "kernel_configs", "*", "*.json")))
    assert len(files) == 6 + 35
    overflowing = 0
    for f in files:
        d = json.load(open(f))
        p = d["properties"]
        w = h if p.get("arrayType") == "ragged" else widest // abs(int(p.get("splitSize", -1)))
        exprs = [a["size"] for a in d["inputArgs"] + d["tempGlobals"] + d["tempLocals"] + [d["outputArg"]]]
        sizes = {"v_MWidthC_1": w, "v_MHeight_2": h, "v_VLength_3": h}
        for e, got in zip(exprs, evaluate(exprs, w, h, h)):
            try:
                exact = int(eval(e, {"__builtins__": {}}, sizes))
            except Exception:
                exact = None                                  # "?"
            fits = exact is not None and -2 ** 31 <= exact < 2 ** 31
            overflowing += exact is not None and not fits
            assert got == (exact if fits else 0), (f, e, got, exact)
    assert overflowing > 0                                    # (else the evaluator's range check would be untested here)


# ---- the same files through the sanitizer build of the self-test ---------------------------------------------------

def probe(exe, path, e, n, env=None):
    full = {k: v for k, v in os.environ.items() if k not in ("SH_CSR_CACHE", "SH_NO_TRUNCATE")}
    full.update({"SH_QUIET_TIMERS": "1", "SH_LOG_LEVEL": "1", "ASAN_OPTIONS": "detect_leaks=0", "OMP_NUM_THREADS": str(THREADS)})
    full.update(env or {})
    r = subprocess.run([os.path.join(HOST, "bin", exe), "--load", path, str(e), str(n)], capture_output=True, text=True, env=full,
                       timeout=300)
    return r.returncode, [l for l in r.stdout.splitlines() if l.startswith("LOAD ")], r.stderr


def test_every_file_under_the_sanitizer_build(files, tmp_path):
    """bin/host_selftest_san is the self-test and the library's sources in one executable under AddressSanitizer and
    UBSan.  Its --load does what sh_mm_load_ex does and then runs Gold<T>::spmv over the rows: no report, the exit
    status of the ordinary build, the same checksums.  The self-test's own body runs once under it too."""
    subprocess.check_call(["make", "-s", "-C", HOST, "selftest-san"], stderr=subprocess.DEVNULL)

    def clean(err):
        return "AddressSanitizer" not in err and "runtime error:" not in err

    (tmp_path / "st").mkdir()
    r = subprocess.run([os.path.join(HOST, "bin", "host_selftest_san"), str(tmp_path / "st")], capture_output=True, text=True,
                       env={**os.environ, "SH_QUIET_TIMERS": "1", "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and "all passed" in r.stdout and clean(r.stderr), (r.stdout[-400:], r.stderr[-800:])

    for name, path in files["paths"].items():
        if name == "special_values":
            continue
        refused = name in REFUSED or files["big"].get(name, (None,))[0] is not None
        combos = COMBOS if not name.startswith("big_") else [(0, 1), (1, 2)]     # (2.5 MB each: PageRank on float, SCC on int)
        for e, n in combos:
            code, line, err = probe("host_selftest_san", path, e, n)
            assert clean(err), (name, e, n, err[-1200:])
            assert code == (255 if refused else 0), (name, e, n, code, err[-400:])
            if not refused:
                assert line and line == probe("host_selftest", path, e, n)[1], (name, e, n)

    # the cache cases: a valid cache file written by the ordinary build, damaged, read by the sanitizer build
    import shutil
    src = tmp_path / "m.mtx"
    shutil.copyfile(mtx("matrix5"), src)
    cache = tmp_path / "cache"
    cache.mkdir()
    env = {"SH_CSR_CACHE": str(cache)}
    for e, suffix in ((0, "f32"), (1, "i32")):
        fresh = probe("host_selftest", str(src), e, 0)
        assert fresh[0] == 0 and probe("host_selftest", str(src), e, 0, env)[1] == fresh[1]
        p = cache / ("m.mtx.shcsr." + suffix)
        valid = p.read_bytes()
        for what, blob in damaged_caches(valid).items():
            p.write_bytes(blob)
            code, line, err = probe("host_selftest_san", str(src), e, 0, env)
            assert clean(err) and code == 0 and line == fresh[1], (what, code, err[-1200:])
            assert p.read_bytes() == valid, what                                 # parsed again, cache rewritten
        code, line, err = probe("host_selftest_san", str(src), e, 0, env)         # and a sound cache is read soundly
        assert clean(err) and code == 0 and line == fresh[1]
