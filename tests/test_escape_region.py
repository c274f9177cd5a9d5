"""Host check of the escape table keyed by sub-brick regions (csrc/escape.h
EscShape, esc_compute_region; tests/cpp/escape_region_check.cpp): random
anisotropic grids (8^3, 12 x 5 x 9, 16 x 16 x 4 among them) of blobs and
planes, eight region shapes, over 10^5 rays per shape walked with the
kernels' f32 DDA, the table asked once per 4^3 brick entered for the region
of the cell the walk is in."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_cache = {}


def _results(tmp_path_factory):
    if "res" not in _cache:
        exe = tmp_path_factory.mktemp("escreg") / "escregchk"
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off",
                        "-I", os.path.join(ROOT, "zig_raytracing_contest_amd", "csrc"),
                        "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "escape_region_check.cpp"), "-o", str(exe)],
                       check=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
        rows = [json.loads(line) for line in r.stdout.splitlines()]
        print(r.stdout)
        _cache["res"] = (r.returncode, rows, r.stderr)
    return _cache["res"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_escape_regions_are_sound(tmp_path_factory):
    rc, rows, err = _results(tmp_path_factory)
    assert rows[0] == {"key_fails": 0}, rows[0]
    shapes = rows[1:]
    assert [tuple(s["shape"]) for s in shapes][:4] == [(4, 4, 4), (2, 2, 2), (1, 1, 1), (1, 4, 1)]
    for s in shapes:
        assert s["rays"] >= 100000, s
        # (a) no occupied cell after an escape point, and the table fires
        assert s["unsound"] == 0, s
        assert s["escapes"] > 10000 and s["steps_after_escape"] > 50000, s
        # (b) a region's bit is set wherever its brick's bit is; regions past
        # the grid's edge (clipped away entirely) hold no bit
        assert s["subset_fails"] == 0, s
        # (c) the brick shape is esc_compute's table
        assert s["brick_diff"] == 0, s
    assert sum(s["clipped_regions"] for s in shapes) > 1000
    # finer regions set more bits and end more walks than the brick's
    brick = shapes[0]
    for s in shapes[1:]:
        assert s["bits_set"] > brick["bits_set"] and s["escapes"] > brick["escapes"], (s, brick)
    # the check can fail: tables built for each region's first cell alone
    # (a start box too small for the rays it is asked for) are caught
    for s in shapes:
        if tuple(s["shape"]) != (1, 1, 1):
            assert s["control_first_cell"] > 100, s
    assert rc == 0, err


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_no_dilation_control_finds_violations(tmp_path_factory):
    """The same walks over tables built WITHOUT the one-cell dilation must
    visit an occupied cell after an escape point.  The walks that do are rare:
    face-tie rays through cell corners of nearly cubic cells, from origins so
    far away that their f32 crossing times swap two crossings the slope margin
    does not cover (the check's header has the arithmetic).  The grids and ray
    classes that hold them are part of every shape's run, so the proof's table
    is held to zero violations on the very walks that break the control's."""
    rc, rows, err = _results(tmp_path_factory)
    counts = [s["control_no_dilation"] for s in rows[1:]]
    print(counts)
    assert sum(counts) > 0, counts
    assert all(s["unsound"] == 0 for s in rows[1:])
