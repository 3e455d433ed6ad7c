"""The phase-1 work items of the x-tiled plan on the device: with the end of every XCD's list re-cut (the default) and
plain (SH_P1_TAIL=0), on the shapes of tests/test_p1_items_cpu.py, all four semirings give the same bits as each other
and as the oracle's gold, through the host-built and the device-built layout; and both builders give the same arrays."""
import ctypes as C

import numpy as np
import pytest

import p1_items_shapes as S
from test_builder_gpu import compare, tools   # noqa: F401  (the tools build's engine and sh_debug_compare_builds)

pytestmark = pytest.mark.gpu


def tail_env(monkeypatch, on):
    if on:
        monkeypatch.delenv("SH_P1_TAIL", raising=False)
    else:
        monkeypatch.setenv("SH_P1_TAIL", "0")


@pytest.mark.parametrize("name", sorted(S.SHAPES))
def test_semirings_with_and_without_the_tail_policy(monkeypatch, name):
    from oracle import oracle as O
    from sparseharness_amd.engine import Engine
    rows, cols, rp, ci, va = S.matrix(name)
    vi = va.astype(np.int32)
    with Engine(0) as eng:
        mats = {}   # (tail, builder, integer) -> matrix; the switch is read when a matrix is uploaded
        for tail in (False, True):
            tail_env(monkeypatch, tail)
            for build in (1, 2):
                mats[tail, build, False] = eng.upload_csr(rows, cols, rp, ci, va, plan=2, build=build)
                mats[tail, build, True] = eng.upload_csr(rows, cols, rp, ci, vi, plan=2, build=build)
                assert mats[tail, build, False].plan()[0] == "tiled"
                assert mats[tail, build, False].builder()[0] == ("host" if build == 1 else "device")
            assert mats[tail, 1, False].describe() == mats[tail, 2, False].describe()
        for sem in (O.PLUS_TIMES_F32, O.MIN_PLUS_F32, O.OR_AND_I32, O.MAX_MIN_I32):
            integer = sem in (O.OR_AND_I32, O.MAX_MIN_I32)
            dt = np.int32 if integer else np.float32
            xs = (np.arange(cols) % 3 == 0).astype(np.int32) if integer else S.x_float(cols)
            ys = (np.arange(rows) % 5).astype(dt)
            alpha, beta = {O.PLUS_TIMES_F32: (1.0, 0.5), O.MIN_PLUS_F32: (0.0, 0.0), O.OR_AND_I32: (1, 1), O.MAX_MIN_I32: (1, 1)}[sem]
            want = O.kernel(sem, rp, ci, vi if integer else va, xs, ys, alpha, beta)
            xv, yv, out = eng.vector(xs), eng.vector(ys), eng.alloc(rows)
            for tail in (False, True):
                for build in (1, 2):
                    out.upload(np.full(rows, 77, dt))
                    eng.spmv(sem, mats[tail, build, integer], xv, yv, alpha, beta, out)
                    got = out.download(dt)
                    np.testing.assert_array_equal(got.view(np.uint32), np.asarray(want, dt).view(np.uint32),
                                                  err_msg=f"{name} semiring {sem} tail {tail} build {build}")
        for m in mats.values():
            m.free()


@pytest.mark.parametrize("name", sorted(S.SHAPES))
def test_both_builders_give_the_same_arrays(tools, monkeypatch, name):   # noqa: F811
    rows, cols, rp, ci, va = S.matrix(name)
    for tail in (False, True):
        tail_env(monkeypatch, tail)
        rc, report = compare(tools, rows, cols, rp, ci, va)
        assert rc == 0, (name, tail, rc, report)
