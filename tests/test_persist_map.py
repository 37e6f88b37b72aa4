"""The tile queue of the persistent level-0 loop (rray_amd/csrc/persist_map.hpp) on the host: the header the kernels
include is compiled with g++ and every (tile count, heads) case is enumerated — the tickets below each head's count name
every tile exactly once, and a ticket at or past the count is refused."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rray_amd", "csrc")
TILES = (1, 15, 64, 32400, 129600)
HEADS = (1, 8, 32, 256)


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("persist") / "persist_map_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC,
                    os.path.join(HERE, "native", "persist_map_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        n, H, *rest = (int(x) for x in line.split())
        table[(n, H)] = rest
    return table


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("n", TILES)
def test_tickets_enumerate_every_tile_once(rows, n, H):
    tiles_hit, doubles, refused_below, accepted_past, count_sum = rows[(n, H)]
    assert count_sum == n, "the heads' counts add up to the tiles"
    assert tiles_hit == n and doubles == 0, "every tile exactly once"
    assert refused_below == 0, "no ticket below a head's count is refused"
    assert accepted_past == 0, "every ticket at or past the count is refused"


def test_every_case_ran(rows):
    assert set(rows) == {(n, H) for n in TILES for H in HEADS}
