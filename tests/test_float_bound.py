"""What keeps tests/test_float_gpu.py honest, checked without a GPU:
  1. the sequential float32 oracle stays inside float_ref.bound() on every input the GPU tests use (so the bound is not
     asking for more than float32 can give on that data),
  2. the bound has teeth: the same oracle fed values, or x, carried in 16 bits falls outside it on most rows,
  3. the device code of the (+,x) kernels, compiled with the Makefile's own flags, holds no fused multiply-add and
     every kernel keeps float32 denormals.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import float_ref as F
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparseharness_amd", "csrc")


def clustered_matrix(n=60_000, seed=11):
    from test_parity_gpu import clustered_matrix as cm   # (imported late: that module opens no device by itself)
    return cm(n, seed)


GENERATORS = {
    "ragged": F.gen_ragged,
    "clustered": lambda: F.gen_clustered(clustered_matrix),
    "wide": F.gen_wide,
    "few16": lambda: F.gen_few_values(16),
    "few255": lambda: F.gen_few_values(255),
    "few4000": lambda: F.gen_few_values(4000),
}


@pytest.fixture(scope="module", params=list(GENERATORS))
def data(request):
    c = GENERATORS[request.param]()
    c["name"] = request.param
    return c


def oracle_out(c, va, x, alpha, beta, y):
    yy = np.zeros(c["rows"], np.float32) if y is None else y
    return O.kernel(O.PLUS_TIMES_F32, c["rp"], c["ci"], va, x, yy, alpha, beta, vlength=c["cols"])


def test_ragged_has_the_row_lengths_it_promises():
    c = F.gen_ragged()
    deg = np.diff(c["rp"])
    assert set(F.RAGGED_LENGTHS) <= set(deg.tolist())
    assert (c["ci"] < 0).any() and (c["ci"] >= c["cols"]).any()
    assert np.count_nonzero(c["ci"] == 1234) > 0.04 * len(c["ci"])
    assert (c["va"] < 0).any() and (c["va"] > 0).any() and (c["x"] < 0).any()


def test_few_values_have_the_counts_they_promise():
    for k in (16, 255, 4000):
        va = F.gen_few_values(k)["va"]
        words = np.unique(va.view(np.uint32))
        assert len(words) == k and np.isfinite(va).all() and (va != 0).all() and (va < 0).any()


def test_sequential_float32_oracle_is_inside_the_bound(data):
    c = data
    dot, mag, n = F.exact_rows(c["rp"], c["ci"], c["va"], c["x"], c["cols"])
    for alpha, beta, with_y in F.EPILOGUES:
        y = c["y"] if with_y else None
        got = oracle_out(c, c["va"], c["x"], alpha, beta, y)
        F.assert_within(got, dot, mag, n, alpha, y, beta, what=f"oracle {c['name']} alpha={alpha:g} beta={beta:g}")


@pytest.mark.parametrize("narrow", list(F.NARROWINGS))
@pytest.mark.parametrize("what", ["values", "x"])
def test_bound_catches_sixteen_bit_floats(data, what, narrow):
    """The reference stays the full-precision float64 result; only the oracle's input is narrowed."""
    c = data
    dot, mag, n = F.exact_rows(c["rp"], c["ci"], c["va"], c["x"], c["cols"])
    va = F.NARROWINGS[narrow](c["va"]) if what == "values" else c["va"]
    x = F.NARROWINGS[narrow](c["x"]) if what == "x" else c["x"]
    for alpha, beta, with_y in F.EPILOGUES[:2]:
        y = c["y"] if with_y else None
        r = F.ratios(oracle_out(c, va, x, alpha, beta, y), dot, mag, n, alpha, y, beta)
        outside, nonempty = int(np.count_nonzero(r[n > 0] > 1.0)), int(np.count_nonzero(n > 0))
        print(f"[float bound] {c['name']} {what} as {narrow}, alpha={alpha:g}: {outside} of {nonempty} non-empty rows outside")
        assert 2 * outside > nonempty


# ------------------------------------------------------------------ the device code
FUSED = re.compile(r"\bv_(?:pk_)?(?:fma|fmac|mad|mac)_(?:legacy_)?f32\w*")


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    """engine.hip as gfx950 assembly under the flags `make` builds the library with (asked of make, not restated here)."""
    if shutil.which("make") is None:
        pytest.skip("no make")
    r = subprocess.run(["make", "-s", "-C", CSRC, "--eval=__float_bound_flags: ; @echo $(HIPCC) $(FLAGS)", "__float_bound_flags"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cmd = r.stdout.split()
    if not (os.path.exists(cmd[0]) or shutil.which(cmd[0])):
        pytest.skip("no hipcc: the static check of the device code needs the ROCm compiler")
    assert any(a.startswith("--offload-arch=gfx950") for a in cmd), cmd
    out = tmp_path_factory.mktemp("float_bound") / "engine.s"
    flags = [a for a in cmd[1:] if a not in ("-shared", "-fPIC")]
    r = subprocess.run([cmd[0]] + flags + ["-S", "--cuda-device-only", "engine.hip", "-o", str(out)], cwd=CSRC,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out.read_text()


def functions_of(asm):
    """name -> body for every function of the assembly (`name:  ; @name` .. `.Lfunc_end`)."""
    out = {}
    for m in re.finditer(r"^([A-Za-z_$][\w$.]*):\s*; @\1\s*$(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S):
        out[m.group(1)] = m.group(2)
    return out


def test_plus_times_kernels_hold_no_fused_multiply_add(device_asm):
    """-ffp-contract=off is what keeps mul and add two roundings (parity rules): without it hipcc contracts
    acc + x * v into v_fmac_f32 and integer-valued data could not tell.  Integer mads (address arithmetic) are not matched."""
    fns = {k: v for k, v in functions_of(device_asm).items() if "PlusTimesF32" in k}
    names = " ".join(fns)
    for kernel in ("spmv_csr_kernel", "spmv_long_fixup", "spmv_heavy_fixup", "spmv_tiled_phase1", "spmv_tiled_phase2s",
                   "spmm_csr_kernel", "spmm_long_fixup"):
        assert kernel in names, f"no (+,x) instantiation of {kernel} in the assembly"
    bad = {k: sorted(set(FUSED.findall(v))) for k, v in fns.items() if FUSED.search(v)}
    print(f"[float bound] {len(fns)} (+,x) functions scanned, {len(bad)} with a fused multiply-add")
    assert not bad, bad
    for k, v in fns.items():   # (the scan saw the arithmetic it is about)
        if "spmm_csr_kernel" in k or "spmv_csr_kernel" in k:
            assert re.search(r"\bv_(?:pk_)?mul_f32", v) and re.search(r"\bv_(?:pk_)?add_f32", v), k


def test_every_kernel_keeps_float32_denormals(device_asm):
    blocks = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)(.*?)^\s*\.end_amdhsa_kernel", device_asm, re.M | re.S)
    assert len(blocks) > 50
    for name, body in blocks:
        m = re.search(r"\.amdhsa_float_denorm_mode_32\s+(\d+)", body)
        assert m and m.group(1) == "3", (name, m and m.group(0))
