"""Host check of the direction-aware escape table (csrc/escape.h
esc_dir_occupied, esc_ray_usable; tests/cpp/escape_dir_check.cpp): five
anisotropic grids (8^3, 12 x 5 x 9, 16 x 16 x 4, 16^3, 10 x 7 x 13) of a few
hundred triangles, over 10^5 rays each (half of them bounce rays from a
triangle's surface inside an occupied cell), every ray binned with its
reciprocal moved by -2 .. +2 ulp and the table asked in every cell the
sequential traceRay visits, its start cell included; then sixteen grids that
hold one control triangle each."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_cache = {}


def _results(tmp_path_factory):
    if "res" not in _cache:
        exe = tmp_path_factory.mktemp("escdir") / "escdirchk"
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off",
                        "-I", os.path.join(ROOT, "zig_raytracing_contest_amd", "csrc"),
                        "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "escape_dir_check.cpp"), "-o", str(exe)],
                       check=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
        rows = [json.loads(line) for line in r.stdout.splitlines()]
        print(r.stdout)
        _cache["res"] = (r.returncode, rows, r.stderr)
    return _cache["res"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_direction_aware_table_is_sound(tmp_path_factory):
    rc, rows, err = _results(tmp_path_factory)
    scenes = [r for r in rows if r["kind"] == 0]
    assert [tuple(r["grid"]) for r in scenes] == [(8, 8, 8), (12, 5, 9), (16, 16, 4), (16, 16, 16), (10, 7, 13)]
    for r in rows:
        # a truncated walk returns the full walk's (t, u, v, ref); no cell after
        # an escape point holds a ref whose determinant test passes
        assert r["unsound_result"] == 0 and r["unsound_lemma"] == 0, r
        # every bit of the plain table is set in the direction-aware one
        assert r["subset_fails"] == 0, r
        # a direction outside bfc_dir_ok never uses a bit
        assert r["outside_used"] == 0, r
    for r in scenes:
        assert r["rays"] >= 100000 and r["refs"] >= 300, r
        assert r["outside"] > 1000 and r["moved_bins"] > 1000 and r["hits"] > 5000, r
        assert r["bits_dir"] > r["bits_plain"] and r["escapes"] > 10000, r
        # not vacuous: surface-start rays, all of them in occupied cells, of
        # which at least a fifth are ended in their start cell
        assert r["surface_rays"] >= 50000 and r["surface_in_occupied_cell"] == r["surface_rays"], r
        assert r["surface_ended_at_start"] >= 0.2 * r["surface_rays"], r
    assert rc == 0, err


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_controls_find_violations(tmp_path_factory):
    """The same walks over a table built with the cull margin at 0, and over
    one built with unwidened cull cones, must break the proof's lemma (a ref
    whose f32 determinant passes, after an escape point); the unwidened cones
    also change results: their rays graze the wall that table skips and hit
    it.  The proof's table is held to zero on those very walks (above)."""
    rc, rows, err = _results(tmp_path_factory)
    margin = sum(r["control_margin_lemma"] for r in rows)
    cone = sum(r["control_cone_lemma"] for r in rows)
    cone_res = sum(r["control_cone_result"] for r in rows)
    print(margin, cone, cone_res)
    assert margin > 0 and cone > 0 and cone_res > 0
