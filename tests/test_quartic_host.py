"""quartic.inc (roots 0.0.8's analytical solvers as the torus kernel runs them) compiled for the host, against the
oracle's find_roots (its own restatement of the crate), bit for bit.

The inputs are the coefficient sets torus.rs:37-95 forms for the torus batteries' object-space rays (tests/shape_rays.py:
axis rays, in-plane rays, rim and top tangents, origins inside the tube, minor radii 1e-3 to 1.5, direction lengths
1e-3 to 1e3) and the solver's own edge cases: biquadratics, multiple roots, a tiny or zero leading coefficient,
all-zero lower coefficients.  Both sides are built with -ffp-contract=off and share the transcendentals' rounding
(host_libm.inc restates glibc's), so no input is excepted."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import shape_rays as S  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def torus_coefficients(o, d, r):
    """torus.rs:37-95 as leaf_intersect forms it (device_core.inc RR_TORUS)"""
    sd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    e = o[0] * o[0] + o[1] * o[1] + o[2] * o[2] - r * r + 1.0
    f = o[0] * d[0] + o[1] * d[1] + o[2] * d[2] + 0.0
    return (sd * sd, 4.0 * sd * f, 2.0 * sd * e + 4.0 * f * f - 4.0 * (d[0] * d[0] + d[1] * d[1]),
            4.0 * e * f - 2.0 * 4.0 * (o[0] * d[0] + o[1] * d[1]), e * e - 4.0 * (o[0] * o[0] + o[1] * o[1]))


def inputs():
    sets = []
    for r in S.TORUS_RADII:
        R = S.torus_rays(r, np.random.default_rng(int(r * 1000)))
        sets += [torus_coefficients([float(x) for x in o], [float(x) for x in d], r) for o, d in zip(R.o, R.d)]
    n_torus = len(sets)
    sets += [(1.0, 0.0, -5.0, 0.0, 4.0), (1.0, 0.0, 5.0, 0.0, 4.0), (2.0, 0.0, -4.0, 0.0, 2.0), (1.0, 0.0, 0.0, 0.0, -1.0),
             (1.0, 0.0, -2.0, 0.0, 1.0), (3.0, 0.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0, 0.0),  # biquadratics
             (1.0, -4.0, 6.0, -4.0, 1.0), (1.0, -5.0, 9.0, -7.0, 2.0), (1.0, -6.0, 13.0, -12.0, 4.0),  # (x-1)^4, ^3, ^2(x-2)^2
             (1.0, -10.0, 35.0, -50.0, 24.0), (1.0, 2.0, 3.0, 4.0, 5.0), (1.0, 0.0, 1.0, 1.0, 0.0), (1.0, 1.0, 0.0, 0.0, 0.0),
             (1.0, 0.0, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, 1.0, 1.0), (1.0, 0.0, -3.0, 2.0, 0.0), (2.0, -8.0, 0.0, 0.0, 0.0),
             (0.0, 1.0, -6.0, 11.0, -6.0), (0.0, 0.0, 1.0, -3.0, 2.0), (0.0, 0.0, 0.0, 2.0, -1.0), (0.0, 0.0, 0.0, 0.0, 0.0),
             (0.0, 0.0, 0.0, 0.0, 1.0), (0.0, 2.0, 0.0, -3.0, 1.0), (0.0, 1.0, 3.0, 3.0, 1.0), (0.0, 1.0, -3.0, 0.0, 4.0),
             (1e-300, 1.0, -6.0, 11.0, -6.0), (1e-12, -4.0, 6.0, -4.0, 1.0), (1e-12, 0.0, -5.0, 0.0, 4.0),  # a4 tiny
             (1e-24, 4e-18, 2e-12, 4e-6, 1.0), (1e12, -1e13, 3.5e13, -5e13, 2.4e13), (1.0, 1e-8, -2.0, 1e-8, 1.0)]
    rng = np.random.default_rng(8)
    for _ in range(400):  # generic quartics, from their roots and at random
        x = rng.uniform(-3, 3, 4)
        if rng.random() < 0.5:
            x[1] = x[0]
        p = np.poly(x) * rng.choice([1.0, 2.0, 1e-3, 37.0])
        sets.append(tuple(float(c) for c in p))
        sets.append(tuple(float(c) for c in rng.standard_normal(5) * [1, 1, 3, 3, 1]))
    return sets, n_torus


@pytest.fixture(scope="module")
def solved(tmp_path_factory, oracle_mod):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("quartic") / "quartic_check")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", os.path.join(HERE, "native", "quartic_check.cpp"),
                    "-o", exe], check=True)
    sets, n_torus = inputs()
    text = "".join(" ".join(float(c).hex() for c in s) + "\n" for s in sets)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(sets)
    mine = [[float.fromhex(t) for t in line.split()[1:]] for line in out]
    assert all(int(line.split()[0]) == len(m) for line, m in zip(out, mine))
    return sets, n_torus, mine, [oracle_mod.Oracle.find_roots(*s) for s in sets]


def test_roots_equal_the_oracle_bit_for_bit(solved):
    sets, n_torus, mine, want = solved
    bad = [(s, a, b) for s, a, b in zip(sets, mine, want) if [x.hex() for x in a] != [x.hex() for x in b]]
    for s, a, b in bad[:10]:
        print(f"coefficients {s}: quartic.inc {a} oracle {b}")
    assert not bad, f"{len(bad)} of {len(sets)} coefficient sets differ"


def test_the_inputs_reach_every_root_count(solved):
    sets, n_torus, mine, want = solved
    assert n_torus >= 500
    assert {len(w) for w in want[:n_torus]} >= {0, 2, 4} and {len(w) for w in want} == {0, 1, 2, 3, 4}
    assert all(np.isfinite(s).all() for s in sets)
