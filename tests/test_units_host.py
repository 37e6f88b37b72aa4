"""The unit table of rray_amd/build.py (UNITS, unit_command): which device units the build holds, how each is flagged,
and that every kernel-variant row compiles the file and the defines its name states.  No GPU, no compile."""
import os
import re

from rray_amd import build as B

T = ["-mllvm", "-amdgpu-use-amdgpu-trackers=1"]
L = ["-mllvm", "-disable-machine-licm"]
FLAGS = {"-": [], "T": T, "L": L, "TL": T + L}
# every .hip unit of the build and its per-unit flags, written out: a unit that appears, vanishes or changes its flags
# changes the device code of the product (chain, tree and persist spill with machine LICM)
UNITS = """
render.hip -
render_adapt.hip -
render_chain_g0_gl.hip L
render_chain_g0_lds.hip L
render_chain_g1_gl.hip L
render_chain_g1_lds.hip L
render_chain_g2_gl.hip L
render_chain_g2_lds.hip L
render_hit_g0_gl.hip -
render_hit_g0_lds.hip -
render_hit_g1_gl.hip -
render_hit_g1_lds.hip -
render_hit_g2_gl.hip -
render_hit_g2_lds.hip -
render_levels_g0_gl.hip T
render_levels_g0_lds.hip -
render_levels_g1_gl.hip -
render_levels_g1_lds.hip -
render_levels_g2_gl.hip -
render_levels_g2_lds.hip -
render_listed_chain_g0_gl.hip L
render_listed_chain_g0_lds.hip L
render_listed_chain_g1_gl.hip L
render_listed_chain_g1_lds.hip L
render_listed_chain_g2_gl.hip L
render_listed_chain_g2_lds.hip L
render_listed_levels_g0_gl.hip T
render_listed_levels_g0_lds.hip -
render_listed_levels_g1_gl.hip -
render_listed_levels_g1_lds.hip -
render_listed_levels_g2_gl.hip -
render_listed_levels_g2_lds.hip -
render_listed_tree_g0_gl.hip L
render_listed_tree_g0_lds.hip L
render_listed_tree_g1_gl.hip L
render_listed_tree_g1_lds.hip L
render_listed_tree_g2_gl.hip L
render_listed_tree_g2_lds.hip L
render_persist_g0_gl.hip TL
render_rays.hip -
render_tree_g0_gl.hip L
render_tree_g0_lds.hip L
render_tree_g1_gl.hip L
render_tree_g1_lds.hip L
render_tree_g2_gl.hip L
render_tree_g2_lds.hip L
render_views.hip -
render_views_chain_g0_gl.hip L
render_views_chain_g0_lds.hip L
render_views_chain_g1_gl.hip L
render_views_chain_g1_lds.hip L
render_views_chain_g2_gl.hip L
render_views_chain_g2_lds.hip L
render_views_hit_g0_gl.hip -
render_views_hit_g0_lds.hip -
render_views_hit_g1_gl.hip -
render_views_hit_g1_lds.hip -
render_views_hit_g2_gl.hip -
render_views_hit_g2_lds.hip -
render_views_levels_g0_gl.hip T
render_views_levels_g0_lds.hip -
render_views_levels_g1_gl.hip -
render_views_levels_g1_lds.hip -
render_views_levels_g2_gl.hip -
render_views_levels_g2_lds.hip -
render_views_tree_g0_gl.hip L
render_views_tree_g0_lds.hip L
render_views_tree_g1_gl.hip L
render_views_tree_g1_lds.hip L
render_views_tree_g2_gl.hip L
render_views_tree_g2_lds.hip L
"""
EXPECT = dict(line.split() for line in UNITS.strip().splitlines())
VARIANT = re.compile(r"render_(listed_|views_|)(levels|chain|tree|hit)_g([012])_(lds|gl)\.hip$")


def test_the_device_units_are_the_listed_ones():
    assert len(EXPECT) == 71
    hip = [u for u in B.SOURCES if u.endswith(".hip")]
    assert len(hip) == len(set(hip)) and set(hip) == set(EXPECT)
    assert set(B.UNITS) <= set(hip)


def test_every_unit_has_its_recorded_flags():
    for u, code in EXPECT.items():
        assert B.UNITS.get(u, (u, [], []))[2] == FLAGS[code], u
        cmd, _ = B.unit_command(u, "x.o")
        # and they reach the command: every -mllvm option beyond the ones all device code gets (B.DEVICE)
        mllvm = [b for a, b in zip(cmd, cmd[1:]) if a == "-mllvm" and b not in B.DEVICE]
        assert mllvm == FLAGS[code][1::2], u


def test_variant_rows_compile_what_their_names_state():
    rows = [u for u in EXPECT if VARIANT.match(u)]
    assert len(rows) == 66 and set(rows) == set(B.UNITS) - {"render_persist_g0_gl.hip"}
    for u in rows:
        src, kind, g, lc = VARIANT.match(u).groups()
        f, defines, _ = B.UNITS[u]
        assert f == f"unit_{kind}.hip", u
        want = {"RR_UNIT_G": g, "RR_UNIT_LC": "1" if lc == "lds" else "0",
                "RR_UNIT_SRC": {"": "0", "listed_": "1", "views_": "2"}[src]}
        assert len(defines) == 3 and dict(d.split("=") for d in defines) == want, u
        cmd, path = B.unit_command(u, "x.o")
        assert path == os.path.join(B.CSRC, f) and all("-D" + d in cmd for d in defines), u


def test_rows_name_existing_files_and_no_two_rows_are_the_same_compile():
    seen = {}
    for u in B.SOURCES:
        f, defines, _ = B.UNITS.get(u, (u, [], []))
        assert os.path.isfile(os.path.join(B.CSRC, f)), u
        assert seen.setdefault((f, tuple(sorted(defines))), u) == u, (u, seen[(f, tuple(sorted(defines)))])


def test_a_unit_is_keyed_by_its_source_file():
    """Editing unit_tree.hip rebuilds the tree units and nothing else: the key's file is the row's source."""
    by_file = {}
    for u in B.UNITS:
        by_file.setdefault(B.unit_command(u, "x.o")[1], []).append(u)
    tree = by_file[os.path.join(B.CSRC, "unit_tree.hip")]
    assert len(tree) == 18 and all("_tree_" in u for u in tree)
