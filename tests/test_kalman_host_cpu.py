"""csrc/ss_kalman.h compiled by the HOST compiler against the two CPU references, bit for bit (no GPU needed).

The header holds the thread forms of the device Kalman filter as plain C++; the kernels' wave forms take their noise model and
gain rows from it.  tests/kalman_host_main.cpp wraps it in a stand-alone program (flags in the spirit of oracle/Makefile:
no contraction, hardware fma).  References: oracle.cexact kf_* for xyah (NSA noise, conf), tests/bytetrack_ref.py kf_* for xywh
and for xyah with conf = 0.  Inputs: the generators of tests/test_gpu_stages.py::test_kalman_bit_exact (50 initiates, 70 states
for predict, update and project, the latter also with conf = None), and the same counts for xywh.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import cexact
from strongsort_yolo_amd.config import StrongSortConfig
from tests import bytetrack_ref as bref
from tests.gpu_util import bits_equal
from tests.test_gpu_stages import _states

_HERE = os.path.dirname(os.path.abspath(__file__))
INITIATE, PREDICT, PROJECT, UPDATE = 0, 1, 2, 3
CFG = StrongSortConfig()
WP, WV = CFG.std_weight_position, CFG.std_weight_velocity


@pytest.fixture(scope="module")
def host_kf(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kalman_host") / "kalman_host")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "clang++"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                           os.path.join(_HERE, "kalman_host_main.cpp"), "-o", exe])

    def run(op, xywh, means=None, covs=None, z=None, conf=None):
        n = len(z) if means is None else len(means)
        rec = np.zeros((n, 81))
        rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = op, float(xywh), WP, WV
        if means is not None:
            rec[:, 4:12], rec[:, 12:76] = np.asarray(means), np.asarray(covs).reshape(n, 64)
        if z is not None:
            rec[:, 76:80] = z
        if conf is not None:
            rec[:, 80] = conf
        out = subprocess.run([exe], input=rec.tobytes(), stdout=subprocess.PIPE, check=True).stdout
        out = np.frombuffer(out, np.float64).reshape(n, 92)
        return out[:, :8], out[:, 8:72], out[:, 72:76], out[:, 76:92]

    return run


def _same(got, ref):
    return bits_equal(np.ascontiguousarray(got), np.array(ref, np.float64).reshape(np.shape(got)))


@pytest.fixture(scope="module")
def xyah_cases():
    """test_kalman_bit_exact's inputs, in its order of draws"""
    rng = np.random.default_rng(2)
    z0 = np.c_[rng.uniform(50, 1800, 50), rng.uniform(50, 1000, 50), rng.uniform(0.2, 0.8, 50), rng.uniform(40, 300, 50)]
    means, covs = _states(rng, 70, CFG)
    z = means[:, :4] + rng.normal(0, 2, (70, 4)) * [1, 1, 0.005, 1]
    conf = rng.uniform(0.3, 0.95, 70)
    return z0, means, covs.reshape(70, 64), z, conf


@pytest.fixture(scope="module")
def xywh_cases():
    """the same counts for the xywh filter: states that went through 0..5 predict / update rounds of the reference"""
    rng = np.random.default_rng(3)
    z0 = np.c_[rng.uniform(50, 1800, 50), rng.uniform(50, 1000, 50), rng.uniform(10, 240, 50), rng.uniform(40, 300, 50)]
    means, covs = [], []
    for _ in range(70):
        zz = np.array([rng.uniform(50, 1800), rng.uniform(50, 1000), rng.uniform(10, 240), rng.uniform(40, 300)])
        m, c = bref.kf_initiate(zz, True, WP, WV)
        for _ in range(int(rng.integers(0, 6))):
            m, c = bref.kf_predict(m, c, True, WP, WV)
            m, c = bref.kf_update(m, c, zz + rng.normal(0, 1, 4) * [2, 2, 2, 2], True, WP)
            zz = zz + [3, 1, 0, 0]
        means.append(m); covs.append(c)
    means, covs = np.array(means), np.array(covs)
    z = means[:, :4] + rng.normal(0, 2, (70, 4))
    return z0, means, covs, z


def test_xyah_against_oracle(host_kf, xyah_cases):
    z0, means, covs, z, conf = xyah_cases
    m, c, _, _ = host_kf(INITIATE, False, z=z0)
    ref = [cexact.kf_initiate(v, WP, WV) for v in z0]
    assert _same(m, [r[0] for r in ref]) and _same(c, [r[1] for r in ref])
    m, c, _, _ = host_kf(PREDICT, False, means, covs)
    ref = [cexact.kf_predict(means[i], covs[i].reshape(8, 8), WP, WV) for i in range(70)]
    assert _same(m, [r[0] for r in ref]) and _same(c, [r[1] for r in ref])
    m, c, _, _ = host_kf(UPDATE, False, means, covs, z, conf)
    ref = [cexact.kf_update(means[i], covs[i].reshape(8, 8), z[i], conf[i], WP) for i in range(70)]
    assert _same(m, [r[0] for r in ref]) and _same(c, [r[1] for r in ref])
    for cf in (conf, None):
        _, _, zm, S = host_kf(PROJECT, False, means, covs, conf=cf)
        ref = [cexact.kf_project(means[i], covs[i].reshape(8, 8), 0.0 if cf is None else cf[i], WP) for i in range(70)]
        assert _same(zm, [r[0] for r in ref]) and _same(S, [r[1] for r in ref])


@pytest.mark.parametrize("xywh", [False, True], ids=["xyah_conf0", "xywh"])
def test_against_bytetrack_ref(host_kf, xyah_cases, xywh_cases, xywh):
    z0, means, covs, z = xywh_cases if xywh else xyah_cases[:4]
    m, c, _, _ = host_kf(INITIATE, xywh, z=z0)
    ref = [bref.kf_initiate(v, xywh, WP, WV) for v in z0]
    assert _same(m, [r[0] for r in ref]) and _same(c, [r[1] for r in ref])
    m, c, _, _ = host_kf(PREDICT, xywh, means, covs)
    ref = [bref.kf_predict(list(means[i]), list(covs[i]), xywh, WP, WV) for i in range(70)]
    assert _same(m, [r[0] for r in ref]) and _same(c, [r[1] for r in ref])
    m, c, _, _ = host_kf(UPDATE, xywh, means, covs, z, 0.0)
    ref = [bref.kf_update(list(means[i]), list(covs[i]), z[i], xywh, WP) for i in range(70)]
    assert _same(m, [r[0] for r in ref]) and _same(c, [r[1] for r in ref])
    _, _, zm, S = host_kf(PROJECT, xywh, means, covs, conf=0.0)
    ref = [bref.kf_project(list(means[i]), list(covs[i]), xywh, WP) for i in range(70)]
    assert _same(zm, [r[0] for r in ref]) and _same(S, [r[1] for r in ref])
