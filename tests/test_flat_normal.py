"""The per-node table of planes' world normals (rray_amd/csrc/flat_normal.hpp) against the CPU oracle.

flatten_scene stores, for every plane, the reference's normal_to_world(node, (0, 1, 0)), and the flat fused kernels read
it instead of computing it per pixel.  Here the header is compiled alone with g++ (as the host units
are: no contraction), fed the oracle's own inverses of a seeded list of transforms, and every entry is compared bit for
bit with the oracle's normal_at / normal_to_world of the same plane under the same transforms: identity, scale and
translate (the diagonal dispatch, NF_DIAG), rotations and shears (the full inverse), and one and two group ancestors.
Every case must be equal.

The kernels form the same vector with shortcuts of their own (an NF_DIAG level drops its off-diagonal products, which
can change the sign of a zero; the quotients are a reciprocal and a correction).  The header evaluates that sequence
next to the reference's and marks an entry usable only when both give the same bits, and the kernels read usable
entries only.  The second test checks that mark against the two printed vectors, that the seeded list holds both
outcomes, and that almost every entry is usable (the path would otherwise never run)."""
import math
import os
import random
import shutil
import subprocess

import pytest

from oracle.oracle import Mat, Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rray_amd", "csrc")
NF_IDENT, NF_DIAG = 1, 4


def _chain(*ms):
    """The product that applies ms[0] first (the scene files' transform lists)."""
    out = Mat.identity()
    for m in ms:
        out = Mat.multiply(m, out)
    return out


def _diag(rng):
    s = [rng.choice((0.2, 0.5, 1.0, 2.0, 3.7, 10.0)) * rng.uniform(0.5, 1.5) for _ in range(3)]
    t = [rng.uniform(-20.0, 20.0) for _ in range(3)]
    return _chain(Mat.scale(*s), Mat.translate(*t))


def _general(rng):
    ms = []
    for _ in range(rng.randint(2, 4)):
        k = rng.randrange(4)
        if k == 0:
            ms.append(Mat.rotate(rng.choice("xyz"), rng.uniform(-math.pi, math.pi)))
        elif k == 1:
            ms.append(Mat.shear(*[rng.uniform(-0.8, 0.8) if rng.random() < 0.5 else 0.0 for _ in range(6)]))
        elif k == 2:
            ms.append(Mat.scale(*[rng.uniform(0.3, 4.0) for _ in range(3)]))
        else:
            ms.append(Mat.translate(*[rng.uniform(-9.0, 9.0) for _ in range(3)]))
    ms.append(Mat.rotate(rng.choice("xyz"), rng.uniform(-math.pi, math.pi)))  # never diagonal
    return _chain(*ms)


def _any(rng):
    return rng.choice((_diag, _general, _general, lambda r: Mat.identity()))(rng)


def _cases():
    """[(family, [plane transform, innermost group's, ...])], seeded: 201 cases."""
    rng = random.Random(20240611)
    cases = [("identity", [Mat.identity()])]
    cases += [("diag", [_diag(rng)]) for _ in range(40)]
    cases += [("general", [_general(rng)]) for _ in range(60)]
    cases += [("one_group", [_any(rng), _any(rng)]) for _ in range(50)]
    cases += [("two_groups", [_any(rng), _any(rng), _any(rng)]) for _ in range(50)]
    return cases


def _bits(v):
    return [float(x).hex() for x in v]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """Per case: (family, the table entry and the plane's flags from the header, the oracle's two answers, whether
    the kernels may read the entry, the kernels' own sequence's vector)."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("flat_normal")
    exe = str(tmp / "flat_normal_check")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC,
                    os.path.join(HERE, "native", "flat_normal_check.cpp"), "-o", exe], check=True)
    cases = _cases()
    lines, want = [], []
    for _, chain in cases:
        o = Oracle()
        parent, ids = -1, []
        for m in reversed(chain[1:]):  # outermost group first
            parent = o.add("group", parent, m)
            ids.append(parent)
        plane = o.add("plane", parent, chain[0])
        ids.append(plane)
        words = [str(len(chain))]
        for oid in reversed(ids):  # the plane, then its ancestors, innermost first
            words += _bits(o.inverse_of(oid)[:12])
        lines.append(" ".join(words))
        want.append((o.normal_to_world(plane, (0.0, 1.0, 0.0))[:3], o.normal_at(plane, (0.3, -1.7, 2.9))[:3]))
    path = tmp / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(cases)
    rows = []
    for (family, _), line, w in zip(cases, out, want):
        x, y, z, flags, usable, dx, dy, dz = line.split()
        rows.append((family, [x, y, z], int(flags), _bits(w[0]), _bits(w[1]), int(usable), [dx, dy, dz]))
    return rows


@pytest.mark.parametrize("family", ["identity", "diag", "general", "one_group", "two_groups"])
def test_table_entry_equals_the_oracle_bit_for_bit(results, family):
    rows = [r for r in results if r[0] == family]
    assert rows
    # hex strings of both sides are produced by different printers: compare the values' bits
    bad = [(k, got, n2w, nat) for k, (_, got, _, n2w, nat, _, _) in enumerate(rows)
           if [float.fromhex(g).hex() for g in got] != n2w or n2w != nat]
    assert not bad, f"{len(bad)} of {len(rows)} cases differ, first: {bad[0]}"


def test_cases_reach_every_dispatch(results):
    assert len(results) >= 200
    own = {"identity": NF_IDENT, "diag": NF_DIAG, "general": 0}
    for family, want in own.items():
        assert all(r[2] == want for r in results if r[0] == family), family
    nested = [r[2] for r in results if r[0] in ("one_group", "two_groups")]
    assert {0, NF_IDENT, NF_DIAG} <= set(nested)


def test_an_entry_is_usable_exactly_when_the_kernels_sequence_gives_its_bits(results):
    norm = lambda v: [float.fromhex(x).hex() for x in v]
    for k, (_, got, _, _, _, usable, dev) in enumerate(results):
        assert bool(usable) == (norm(got) == norm(dev)), k
    unusable = [k for k, r in enumerate(results) if not r[5]]
    assert unusable, "the list holds a case in which the diagonal shortcut changes the sign of a zero"
    assert len(unusable) <= len(results) // 20, unusable
