"""A frame's dispatch (rray_amd/csrc/frame_plan.hpp) on the host: the header api.cpp plans every run of the levels with
is compiled with g++ into tests/native/frame_plan_check.cpp, which prints what it decides for the cases below.  The
expectations are written out here, derived by hand from the rules in the header's comments and DESIGN.md — never by
calling the header."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rray_amd", "csrc")

RR_E_ARG, RR_E_LIMIT = -1, -5
LISTED_MSG = "internal: the listed-pixel pass needs one batch of a production kernel family"
PW_MSG = "internal: pixel waves need one chain-kernel batch"
LIMIT_MSG = "recursion queues exceed 2^31 events (lower max_depth)"
# sizeof of the wavefront.hpp records (the check program prints its own)
SIZES = {"Event": 64, "HitRec": 32, "CombRec": 64, "CombExt": 40, "DeepRec": 128}


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("frame_plan") / "frame_plan_check")
    # -Wno-comment: the public header's text names a glob ("csrc/*") inside a comment
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-comment", "-I" + CSRC,
                    os.path.join(HERE, "native", "frame_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        head, _, msg = line.partition(" msg=")
        kind, name, *fields = head.split()
        if kind == "sizes":
            name, fields = "", [name] + fields
        row = {}
        for f in fields:
            k, v = f.split("=")
            row[k] = [int(x) for x in v.split(",")] if "," in v else v if kind == "plan" and k == "family" else int(v)
        row["msg"] = msg
        assert (kind, name) not in table
        table[(kind, name)] = row
    return table


def check(rows, kind, name, **want):
    row = rows[(kind, name)]
    got = {k: row[k] for k in want}
    assert got == want, f"{kind} {name}"


def test_record_sizes_and_constants(rows):
    check(rows, "sizes", "", nseg=1024, deep_from=2, deep_shift=5, max_depth=8, e_arg=RR_E_ARG, e_limit=RR_E_LIMIT,
          **SIZES)


def queue_bytes(caps, ev_a, ev_b, ext):
    """The formula above plan_levels: a pending sum (and its refraction half) and a pending index per event of every
    level with children; a hit record, n1 / n2 and an n1n2 index per event of the widest level; the two event queues."""
    pending = SIZES["CombRec"] + (SIZES["CombExt"] if ext else 0) + 4
    return sum(caps[:-1]) * pending + max(caps) * (SIZES["HitRec"] + 2 * 8 + 4) + (ev_a + ev_b) * SIZES["Event"]


def test_plan_levels(rows):
    # unfused: level d holds nb * k^d events; level d + 1 lands in ev_a when d is even
    caps = [4096, 8192, 16384, 32768]
    check(rows, "levels", "unfused_k2_d3", levels=4, cap=caps, ev_a=32768, ev_b=16384, max_cap=32768,
          bytes=queue_bytes(caps, 32768, 16384, False))
    # fused: 768 events are 3 blocks, one per segment at most: 256 events per segment, 1024 segments
    caps = [768, 262144, 262144]
    check(rows, "levels", "fused_k1_d2", levels=3, cap=caps, seg_cap=[0, 256, 256], ev_a=262144, ev_b=262144,
          max_cap=262144, bytes=queue_bytes(caps, 262144, 262144, False))
    check(rows, "levels", "k0", levels=1, cap=1000, ev_a=0, ev_b=0, max_cap=1000, bytes=queue_bytes([1000], 0, 0, False))
    check(rows, "levels", "ext_k2_d1", levels=2, cap=[64, 128], ev_a=128, ev_b=0, bytes=queue_bytes([64, 128], 128, 0, True))


@pytest.mark.parametrize("name,family,k,levels,zero_lcount", [
    ("flat_opaque", "Level0", 0, 1, 0),
    ("reflective_d5", "Chain", 0, 1, 0),
    ("reflective_d0", "Level0", 1, 1, 0),
    ("fused_levels_d3", "FusedLevels", 1, 4, 1),
    ("tree_d0", "Tree", 0, 1, 0),
    ("tree_d5", "Tree", 0, 1, 0),
    ("transparent_no_tree_d2", "Unfused", 2, 3, 1),
])
def test_family(rows, name, family, k, levels, zero_lcount):
    # 64 x 64 samples in one batch; the queue counters are zeroed only where some level queues or lists anything
    check(rows, "plan", name, family=family, k=k, levels=levels, B=4096, zero_lcount=zero_lcount, err=0)


def test_family_planning_depth_and_padding(rows):
    check(rows, "plan", "reflective_d5", plan_depth=0, pad_children=1)  # the chain runs inside the wave
    check(rows, "plan", "fused_levels_d3", plan_depth=3, pad_children=1, max_cap=262144)
    check(rows, "plan", "tree_d5", plan_depth=0, pad_children=0)  # not fused: no segmented queues to pad
    check(rows, "plan", "transparent_no_tree_d2", plan_depth=2, max_cap=4096 * 4)


@pytest.mark.parametrize("name,wave_avg,pw,direct_avg", [
    ("aa1", 0, 0, 1),
    ("aa2_level0", 1, 0, 1),
    ("aa4_chain", 1, 0, 1),
    ("aa8_level0_d0", 1, 0, 1),
    ("aa2_tree", 1, 0, 1),
    ("aa2_fused_levels", 0, 0, 0),  # secondary rays in queues: samples are not final in their wave
    ("aa2_unfused", 0, 0, 0),
    ("aa2_ragged_13x9", 0, 0, 0),   # 26 x 18 samples: no full tiles
    ("aa2_no_avg", 0, 0, 0),
    ("aa3_chain", 0, 1, 1),
    ("aa3_tree", 0, 1, 1),
    ("aa3_level0", 0, 0, 0),        # pixel waves are the chain / tree kernels'
    ("aa3_chain_no_pw", 0, 0, 0),
    ("aa3_chain_odd_block", 0, 0, 0),
    ("aa3_chain_no_avg", 0, 0, 0),
    ("aa3_chain_over_batch", 0, 0, 0),  # 42 x 30 = 1260 samples against a batch of 1259
])
def test_output_mode(rows, name, wave_avg, pw, direct_avg):
    check(rows, "output", name, wave_avg=wave_avg, pw=pw, direct_avg=direct_avg)


def test_pixel_wave_geometry(rows):
    # W = 14: a band of two rows is 28 pixels, 7 per wave; H = 10: 5 bands
    check(rows, "output", "aa3_chain", pw_wpb=4)
    check(rows, "plan", "pw_14x10", family="Chain", n_tiles=20, pw_n=1280, B=1260, tile_fast=0, err=0)


def test_batch(rows):
    # unfused, k = 2, depth 3: the levels hold 1, 2, 4, 8 x B events — 7 B pending sums of 68 bytes, 8 B hit entries of
    # 52 and 8 B + 4 B queued events of 64: 1660 bytes per sample
    assert queue_bytes([1, 2, 4, 8], 8, 4, False) == 1660
    check(rows, "plan", "batch_fits", B=1000000, err=0)
    # 435159040 = 1660 * 262144: 1000000 -> 499968 (500000 & ~63) -> 249984, the first that fits
    check(rows, "plan", "batch_halves", B=249984, max_cap=8 * 249984, err=0)
    check(rows, "plan", "batch_stops_4096", B=4096, max_cap=32768, err=0)  # nothing fits one byte
    # k = 6, depth 8: 4096 * 6^8 events at the last level
    check(rows, "plan", "batch_limit", err=RR_E_LIMIT, msg=LIMIT_MSG)
    assert 4096 * 6 ** 8 >= 2 ** 31


@pytest.mark.parametrize("name,ok,n_tiles,n_pad,group,pad", [
    ("order_groups", 1, 64, 64, 1, 2),
    ("order_chain", 1, 64, 64, 1, 3),
    ("order_flat", 0, 64, 64, 1, 2),
    ("order_general", 0, 64, 64, 1, 2),
    ("order_two_batches", 0, 64, 64, 1, 2),
    ("order_no_chain_order", 0, 64, 64, 1, 3),
    ("order_group4", 1, 64, 64, 4, 0),
    ("order_9_tiles", 1, 9, 12, 1, 2),
    ("order_9_tiles_group4", 0, 9, 12, 4, 0),      # the group order permutes whole blocks of four tiles
    ("order_pw_270_rows", 1, 148230, 148232, 1, 3),  # 3840 x 270 pixels: 135 bands of 1098 pixel waves
    ("order_ragged", 0, 0, 0, 1, 2),
])
def test_order(rows, name, ok, n_tiles, n_pad, group, pad):
    check(rows, "plan", name, order=ok, n_tiles=n_tiles, n_pad=n_pad, group=group, pad=pad, err=0)


@pytest.mark.parametrize("name,persist", [
    ("persist", 1),
    ("persist_listed", 0),
    ("persist_pw", 0),
    ("persist_ragged", 0),
    ("persist_levels", 0),
    ("persist_two_batches", 0),
    ("persist_second_run", 0),
])
def test_persist_candidate(rows, name, persist):
    check(rows, "plan", name, persist=persist)
    if name != "persist_pw":  # pixel waves outside the chain kernels are refused altogether
        check(rows, "plan", name, err=0)


def test_guards(rows):
    check(rows, "plan", "listed_fused_levels", err=RR_E_ARG, msg=LISTED_MSG)
    check(rows, "plan", "listed_two_batches", err=RR_E_ARG, msg=LISTED_MSG)
    check(rows, "plan", "listed_chain", err=0, msg="")
    check(rows, "plan", "pw_two_batches", err=RR_E_ARG, msg=PW_MSG)
    check(rows, "plan", "persist_pw", err=RR_E_ARG, msg=PW_MSG)


@pytest.mark.parametrize("name,spill,deep_nseg", [
    ("spill", 1, 1),        # 16 blocks of 256 samples: one segment of 32 blocks
    ("spill_1m", 1, 128),   # 4096 blocks
    ("spill_off", 0, 1),
    ("spill_tree", 0, 1),
    ("spill_level0", 0, 1),
    ("spill_aa_wave", 0, 1),
    ("spill_pw", 0, 1),
    ("spill_listed", 0, 1),
    ("spill_depth_1", 0, 1),
])
def test_spill(rows, name, spill, deep_nseg):
    check(rows, "plan", name, spill=spill, deep_nseg=deep_nseg, deep_seg_cap=256 << 5, err=0)


@pytest.mark.parametrize("name,passes,B", [
    # 48 samples a row at aa 3: a unit is lcm(8, 3) = 24 sample rows, 1152 samples
    ("passes_2", 1, 1152),
    ("passes_default", 0, 2304),
    ("passes_8_of_4_units", 1, 1152),  # never less than a unit a pass
    ("passes_part_unit", 0, 1920),     # 40 rows are no whole units
    ("passes_small_batch", 0, 1024),   # a batch below a unit
    ("passes_direct", 0, 2304),        # no canvas to average
])
def test_passes(rows, name, passes, B):
    check(rows, "plan", name, passes=passes, B=B, err=0)
