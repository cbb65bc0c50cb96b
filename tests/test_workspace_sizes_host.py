"""CPU: what every geometry *_workspace_bytes query of the C ABI (revision 602) returns, as a literal table recorded from
the build before csrc/workspace.h carved the layouts (a shape whose regions are no multiples of 256 bytes, the shapes at
each upper limit, and every refusal: 0 in some files, -1 in others); that every entry point with a workspace_bytes
argument refuses a workspace one byte short, before anything is launched; and the carver itself, compiled alone with
the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cloudaae_amd", "libcloudaae_hip.so")

M24, M28, M31 = 1 << 24, 1 << 28, (1 << 31) - 1

# f >= 0 is a frame count of these three (an empty batch returns early); h * w <= 2^24; f * h * w <= 2^28
_FRAMES_COMPONENTS = [((3, 33, 35), 14080), ((0, 1, 1), 256), ((1, 4096, 4096), 67109120), ((16, 4096, 4096), 1073742080),
                      ((M28, 1, 1), 1073742080),
                      ((-1, 1, 1), 0), ((1, 0, 1), 0), ((1, 1, 0), 0), ((1, 4097, 4096), 0), ((17, 4096, 4096), 0)]
# b, wh, ww >= 1; wh * ww <= 2^24; b * wh * ww <= 2^28
_WINDOWS = [((3, 33, 35), 688), ((1, 1, 1), 232), ((1, 4096, 4096), 1867776), ((16, 4096, 4096), 29884416),
            ((M28, 1, 1), 61203283968),
            ((0, 1, 1), 0), ((1, 0, 1), 0), ((1, 1, 0), 0), ((1, 4097, 4096), 0), ((17, 4096, 4096), 0)]

TABLE = {
    "hpr": [((3, 131), 6700), ((1, 5), 100), ((0, 5), 0), ((65535, 13000), 14483497148)],      # (no refusal value)
    "estimate_normals": [((3, 171), 55296), ((1, 1), 17408), ((65535, M28), 9666019328),
                         ((0, 10), -1), ((1, 0), -1), ((1, M28 + 1), -1)],
    "pose_score": [((3, 5, 130), 720), ((1, 1, 1), 16), ((1024, 1024, 2048), 536870912),
                   ((0, 1, 1), -1), ((1, 0, 1), -1), ((1, 1, 0), -1)],
    "cloud_diameter": [((21, 1000), 2688), ((1, 1), 8), ((65536, 32768), 268435456), ((0, 1), -1), ((1, 0), -1)],
    "frame_segments": [((2, 17, 19, 3), 18944), ((1, 1, 1, 0), 3584), ((1, 1 << 14, 1 << 14, 21), 5733615616),
                       ((4096, 256, 256, 1), 5649729536),
                       ((0, 1, 1, 1), -1), ((1, 0, 1, 1), -1), ((1, 1, 0, 1), -1), ((1, 1, 1, -1), -1),
                       ((2, 1 << 14, 1 << 14, 1), -1)],
    "radius_outlier": [((3, 171), 398336), ((1, 0), 132096), ((21, M28), 5648287488),
                       ((0, 10), -1), ((1, -1), -1), ((1, M28 + 1), -1)],
    "ragged_fps": [((171,), 1536), ((0,), 0), ((M28,), 2147483648), ((-1,), -1), ((M28 + 1,), -1)],
    "mesh_weights": [((257,), 5120), ((1,), 1024), ((M28,), 4311744512), ((0,), -1), ((M28 + 1,), -1)],
    "render": [((2, 9, 11, 3, 12, 12), 3072), ((1, 1, 1, 1, 0, 0), 512), ((1, 4096, 4096, 1, 5, 7), 134219008),
               ((16, 4096, 4096, 1, 5, 7), 2147484928), ((1, 1, 1, M31, M31, M31), 42949673472),
               ((1, 1, 1, 1, 0, M24), 67109376),
               ((0, 1, 1, 1, 0, 0), 0), ((1, 0, 1, 1, 0, 0), 0), ((1, 1, 0, 1, 0, 0), 0), ((1, 4097, 4096, 1, 0, 0), 0),
               ((17, 4096, 4096, 1, 0, 0), 0), ((1, 1, 1, 0, 0, 0), 0), ((1, 1, 1, 1, -1, 0), 0),
               ((1, 1, 1, 1, M31 + 1, 0), 0), ((1, 1, 1, 1, 0, -1), 0), ((1, 1, 1, 256, 0, M31 + 1), 0),
               ((1, 1, 1, 1, 0, M24 + 1), 0)],
    "pose_max_dist": [((3, 5, 7), 1680), ((1, 1, 1), 16), ((1024, 1024, 256), 4294967296),
                      ((0, 1, 1), -1), ((1, 0, 1), -1), ((1, 1, 0), -1)],
    "frame_clouds": [((2, 17, 19, 3, 100), 256), ((1, 1, 1, 1, 1), 256), ((1, 4096, 4096, 2047, 1 << 20), 134152192),
                     ((16, 4096, 4096, 1, 1), 65536), ((1, 4096, 4096, 131071, 1), 8589869056),
                     ((0, 1, 1, 1, 1), 0), ((1, 0, 1, 1, 1), 0), ((1, 1, 0, 1, 1), 0), ((1, 1, 1, 0, 1), 0),
                     ((1, 1, 1, 1, 0), 0), ((1, 1, 1, 1, (1 << 20) + 1), 0), ((1, 4097, 4096, 1, 1), 0),
                     ((17, 4096, 4096, 1, 1), 0), ((1, 1, 1, 2048, 1 << 20), 0), ((1, 4096, 4096, 131072, 1), 0)],
    "transform_hausdorff": [((3,), 24), ((1,), 8), ((1 << 20,), 8388608), ((0,), -1), (((1 << 20) + 1,), -1)],
    "depth_components": _FRAMES_COMPONENTS,
    "component_labels": [((3, 33, 35), 41984), ((0, 1, 1), 512), ((1, 4096, 4096), 201327104), ((16, 4096, 4096), 3221225984),
                         ((M28, 1, 1), 4294967808),
                         ((-1, 1, 1), 0), ((1, 0, 1), 0), ((1, 1, 0), 0), ((1, 4097, 4096), 0), ((17, 4096, 4096), 0)],
    "depth_creases": _FRAMES_COMPONENTS,
    "depth_align_step": _WINDOWS,
    "depth_contour_sums": _WINDOWS,
}


@pytest.fixture(scope="module")
def cdll():
    import torch  # noqa: F401  (binds the library to torch's HIP runtime, as the product does)
    from cloudaae_amd import _lib
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    return _lib.lib()._cdll


def test_the_table_names_every_geometry_query():
    import re
    header = open(os.path.join(ROOT, "include", "cloudaae_hip.h")).read()
    declared = set(re.findall(r"\bcloudaae_([a-z0-9_]+)_workspace_bytes\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    training = {"bn", "edgeconv", "mean", "loss_tail"}                  # single double regions of the training path
    assert declared - training == set(TABLE)


@pytest.mark.parametrize("query, args, want", [(q, a, v) for q, rows in TABLE.items() for a, v in rows])
def test_workspace_query(cdll, query, args, want):
    assert getattr(cdll, "cloudaae_%s_workspace_bytes" % query)(*args) == want


_X = 0x1000          # a fake, never dereferenced address (8-byte aligned): every call below must fail in validation

# entry point -> (its query, the query's arguments, the call's arguments in front of (workspace, workspace_bytes, stream),
#                 the refusal's text)
_SMALLER = "workspace smaller than cloudaae_%s_workspace_bytes"
_SMALLER_GN = "the workspace is smaller than cloudaae_%s_workspace_bytes or not 8-byte aligned"
UNDERSIZED = {
    "cloudaae_estimate_normals": ("estimate_normals", (3, 171),
                                  [3, _X, _X, 3, 171, 4, _X, 3, 12, 0.02, 3, None, _X, _X, _X], _SMALLER),
    "cloudaae_frame_segments": ("frame_segments", (2, 17, 19, 3), [2, 17, 19, _X, _X, _X, 3, _X, _X, 0.2, _X, _X, _X], _SMALLER),
    "cloudaae_radius_outlier": ("radius_outlier", (3, 171), [3, _X, _X, 171, 100, 0.02, 512, _X, _X, _X, _X], _SMALLER),
    "cloudaae_ragged_fps": ("ragged_fps", (171,), [3, _X, _X, 171, 16, _X, _X, _X], _SMALLER),
    "cloudaae_mesh_weights": ("mesh_weights", (257,), [1, _X, _X, 100, 257, _X, _X, _X, _X, _X, _X], _SMALLER),
    "cloudaae_render_frames": ("render", (2, 9, 11, 3, 12, 12),
                               [1, _X, _X, 4, 4, _X, _X, 2, 9, 11, _X, _X, 3, _X, _X, _X, _X, _X, 12, 12, 0.1, _X, _X, _X, _X,
                                _X], _SMALLER),
    "cloudaae_frame_clouds": ("frame_clouds", (2, 17, 19, 3, 100),
                              [2, 17, 19, _X, _X, _X, 3, _X, _X, _X, _X, 100, 1, _X, _X, _X, _X], _SMALLER),
    "cloudaae_depth_components": ("depth_components", (3, 33, 35), [3, 33, 35, _X, _X, _X, _X, _X], _SMALLER),
    "cloudaae_depth_creases": ("depth_creases", (3, 33, 35), [3, 33, 35, _X, _X, _X, _X, 3, 1, 0.5, _X, _X, _X, _X], _SMALLER),
    "cloudaae_component_labels": ("component_labels", (3, 33, 35), [3, 33, 35, _X, 1, 8, _X, _X, _X, _X, _X, _X], _SMALLER),
    "cloudaae_depth_align_step": ("depth_align_step", (3, 33, 35),
                                  [1, 40, 40, _X, 3, _X, _X, 33, 35, _X, _X, _X, _X, 0.5, _X, _X, _X, _X, _X, _X], _SMALLER_GN),
    "cloudaae_depth_contour_sums": ("depth_contour_sums", (3, 33, 35),
                                    [1, 40, 40, _X, 3, _X, _X, 33, 35, _X, _X, _X, _X, 2, _X, _X, _X], _SMALLER_GN),
}


def test_every_entry_with_a_workspace_size_is_listed():
    import re
    header = open(os.path.join(ROOT, "include", "cloudaae_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    takers = set(re.findall(r"\bint\s+(cloudaae_[a-z0-9_]+)\s*\([^;]*\blong long workspace_bytes\b[^;]*\)\s*;", text))
    assert takers == set(UNDERSIZED)


@pytest.mark.parametrize("fn", sorted(UNDERSIZED))
def test_a_workspace_one_byte_short_is_refused(cdll, fn):
    from cloudaae_amd import _lib
    query, qargs, args, text = UNDERSIZED[fn]
    need = getattr(cdll, "cloudaae_%s_workspace_bytes" % query)(*qargs)
    assert need > 0
    rc = getattr(_lib.lib(), fn)(*(args + [_X, need - 1, None]))
    assert rc != 0
    assert cdll.cloudaae_last_error().decode() == "%s: %s" % (fn, text % query)


def test_carver_alone_under_sanitizers(tmp_path):
    """cloudaae_amd/csrc/workspace.h with tests/workspace_carver_main.cpp, a program of its own: alignment of every pointer,
    a null base, a region of no elements, a total above 2^32."""
    cxx = shutil.which("g++")
    assert cxx, "no g++ on this machine"
    exe = str(tmp_path / "workspace_carver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "cloudaae_amd", "csrc"),
                    os.path.join(ROOT, "tests", "workspace_carver_main.cpp"), "-o", exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and "workspace carver: ok" in done.stdout, done.stdout + done.stderr
