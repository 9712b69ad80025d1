"""CPU tests of the mesh rasteriser's integer half and of its oracle (no GPU needed).

csrc/raster_fixed.h (snap, orientation, edge functions, top-left rule, clipped pixel box -- the same header the device compiles)
is built for the host only into tests/raster_fixed_check.cpp, a stand-alone program, with AddressSanitizer and UBSan, and run on a
few hundred triangles; every byte of its coverage is compared with the numpy oracle's brute-force test of EVERY pixel of the image
(tests/raster_common.py: Python integers and int64, floor division, no bounding box), exactly.  The triangles: random ones on and
off the 1/256 grid, and the adversarial ones -- corners on pixel centres, edges through pixel centres, slivers between centres that
cover nothing, corners at +-2^20 pixels (the last usable position) and just beyond, boxes clipped on every side of the image, zero
area, a corner behind the near plane or not finite.  Also: engine.vertex_face_csr against a brute-force inversion, and the oracle's
own watertightness -- a closed manifold covers every pixel of its silhouette exactly twice, and two triangles that share an edge
through pixel centres never both own a pixel."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import raster_common as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
W, H = 37, 29
ZNEAR = 0.05


def triangles():
    """[(name, W, H, xy float32 [3, 2], z)]"""
    rng = np.random.RandomState(11)
    out = []
    for i in range(120):                                                # anywhere around the image, any winding
        out.append(("random %d" % i, W, H, rng.uniform(-8.0, 45.0, size=(3, 2)), 1.0))
    for i in range(60):                                                 # small, on the 1/256 grid: exact ties with pixel centres are common
        c = rng.randint(0, 30, size=2) + 0.5
        out.append(("grid %d" % i, W, H, c + rng.randint(-3 * 256, 3 * 256 + 1, size=(3, 2)) / 256.0, 1.0))
    for i in range(40):                                                 # corners ON pixel centres
        out.append(("centres %d" % i, W, H, rng.randint(-2, 40, size=(3, 2)) + 0.5, 1.0))
    for i in range(30):                                                 # an edge through a run of pixel centres: horizontal, vertical, diagonal
        a = rng.randint(2, 12, size=2) + 0.5
        n = rng.randint(3, 12)
        d = [(1, 0), (0, 1), (1, 1), (1, -1), (2, 1), (1, 2)][i % 6]
        b = a + n * np.asarray(d)
        third = a + rng.uniform(-9.0, 9.0, size=2)
        out.append(("edge through centres %d" % i, W, H, np.stack([a, b, third]), 1.0))
    for i in range(20):                                                 # slivers between two rows / columns of centres
        y0 = rng.randint(1, 25) + 0.5
        p = np.array([[1.2, y0 + 0.1], [33.7, y0 + 0.4], [17.0, y0 + 0.9]])
        out.append(("sliver %d" % i, W, H, p if i % 2 == 0 else p[:, ::-1].copy(), 1.0))
    far = 2.0 ** 20
    out += [("far corners", W, H, np.array([[-far, -far], [far, -far], [0.0, far]]), 1.0),
            ("far corners reversed", W, H, np.array([[-far, -far], [0.0, far], [far, -far]]), 1.0),
            ("far diagonal", W, H, np.array([[-far, -far], [far, far], [far, far - 3.0]]), 1.0),
            ("far edge through the image", W, H, np.array([[-far, 10.5], [far, 10.5], [12.0, far]]), 1.0),
            ("beyond far", W, H, np.array([[-far - 1.0, 0.0], [far, 0.0], [0.0, far]]), 1.0),
            ("clipped left and top", W, H, np.array([[-30.0, -20.0], [20.0, 5.0], [4.0, 25.0]]), 1.0),
            ("clipped right and bottom", W, H, np.array([[60.0, 50.0], [10.0, 20.0], [30.0, 2.0]]), 1.0),
            ("clipped on every side", W, H, np.array([[-100.0, -80.0], [200.0, -60.0], [10.0, 300.0]]), 1.0),
            ("wholly off-screen", W, H, np.array([[-30.0, -20.0], [-5.0, -3.0], [-9.0, -25.0]]), 1.0),
            ("zero area", W, H, np.array([[3.0, 3.0], [9.0, 9.0], [6.0, 6.0]]), 1.0),
            ("one pixel wide image", 1, 33, np.array([[-3.0, -3.0], [5.0, 12.0], [-4.0, 40.0]]), 1.0),
            ("behind the near plane", W, H, np.array([[3.0, 3.0], [30.0, 9.0], [6.0, 26.0]]), 0.01),
            ("on the near plane", W, H, np.array([[3.0, 3.0], [30.0, 9.0], [6.0, 26.0]]), ZNEAR),
            ("NaN corner", W, H, np.array([[3.0, np.nan], [30.0, 9.0], [6.0, 26.0]]), 1.0),
            ("infinite corner", W, H, np.array([[3.0, 3.0], [np.inf, 9.0], [6.0, 26.0]]), 1.0),
            ("NaN depth", W, H, np.array([[3.0, 3.0], [30.0, 9.0], [6.0, 26.0]]), np.nan)]
    return out


def test_header_coverage_equals_the_oracle_exactly(tmp_path):
    exe = str(tmp_path / "raster_fixed_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17",
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "raster_fixed_check.cpp"), "-o", exe], check=True)
    cases = triangles()
    assert len(cases) >= 250
    with open(str(tmp_path / "tri.bin"), "wb") as fh:
        for _, w, h, xy, z in cases:
            fh.write(struct.pack("<ii8f", w, h, *np.asarray(xy, np.float32).reshape(6).tolist(), z, ZNEAR))
    r = subprocess.run([exe, str(tmp_path / "tri.bin"), str(tmp_path / "cov.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.strip().splitlines()[-2] == "%d records" % len(cases)
    assert re.fullmatch(r"[1-9]\d* checks, 0 failed", r.stdout.strip().splitlines()[-1])
    blob = open(str(tmp_path / "cov.bin"), "rb").read()
    pos, covered, empty = 0, 0, []
    for name, w, h, xy, z in cases:
        usable, sx0, sx1, sx2, sy0, sy1, sy2, area2, bx0, by0, bx1, by1 = struct.unpack_from("<i3i3iq4i", blob, pos)
        pos += 52
        got = np.frombuffer(blob, np.uint8, w * h, pos).reshape(h, w).astype(bool)
        pos += w * h
        screen = np.concatenate([np.asarray(xy, np.float32), np.full((3, 1), z, np.float32)], 1)
        ox, oy, ok = RC.snap(screen, ZNEAR)
        assert bool(usable) == bool(ok.all()), name
        if not usable:
            assert not got.any(), name
            empty.append(name)
            continue
        assert [sx0, sx1, sx2] == ox.tolist() and [sy0, sy1, sy2] == oy.tolist(), name
        x, y = [int(v) for v in ox], [int(v) for v in oy]
        assert area2 == abs((x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])), name
        assert (bx0, by0, bx1, by1) == RC.pixel_box(x, y, h, w), name
        want = RC.coverage_mask(x, y, h, w)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:8].tolist())
        covered += int(got.sum())
        if not got.any():
            empty.append(name)
    assert pos == len(blob)
    assert covered > 20000
    # what the cases are named after
    for name in ["beyond far", "behind the near plane", "NaN corner", "infinite corner", "NaN depth", "wholly off-screen", "zero area"] + \
            ["sliver %d" % i for i in range(20)]:
        assert name in empty, name
    for name in ("far corners", "far corners reversed", "on the near plane", "clipped on every side", "far edge through the image"):
        assert name not in empty, name


def test_vertex_face_csr_is_the_brute_force_inversion():
    from smplifyx_amd import engine
    rng = np.random.RandomState(3)
    _, ico = RC.icosphere(2)
    rand = rng.randint(0, 40, size=(90, 3))
    rand[5] = [7, 7, 9]                                                 # a face that names a vertex twice: listed once
    for faces, V in ((ico, 162), (rand, 45), (np.array([[2, 1, 0]]), 3)):
        off, vf = engine.vertex_face_csr(faces, V)
        assert off.dtype == np.int32 and vf.dtype == np.int32 and off.shape == (V + 1,) and off[0] == 0 and off[-1] == vf.size
        for v in range(V):
            assert vf[off[v]:off[v + 1]].tolist() == [f for f in range(len(faces)) if v in faces[f]], v
    again = engine.vertex_face_csr(ico[::-1].copy(), 162)
    assert all(np.array_equal(a, b) for a, b in zip(again, engine.vertex_face_csr(ico[::-1].copy(), 162)))
    for bad in (np.array([[0, 1, 5]]), np.array([[0, -1, 2]]), np.zeros((0, 3), np.int64), np.array([0, 1, 2]), np.array([[0.0, 1.0, 2.0]])):
        with pytest.raises(ValueError):
            engine.vertex_face_csr(bad, 5)


def test_oracle_is_watertight_on_a_closed_manifold():
    """Every pixel of an icosphere's silhouette is covered exactly twice (front and back), none once or three times; and the two
    halves of a quad split along a diagonal through pixel centres never both own a pixel."""
    verts, faces = RC.icosphere(2)
    for (hh, ww), t, f in (((53, 75), (0.1, -0.05, 3.0), 60.0), ((120, 160), (0.0, 0.0, 2.2), 150.0)):
        screen = RC.project(verts, t, (f, f), (ww / 2.0, hh / 2.0), dtype=np.float32)
        ras = RC.rasterize(screen, faces, hh, ww)
        assert ras["dropped"] == 0
        counts = np.bincount(ras["hits"].reshape(-1))
        assert counts.size == 3 and counts[1] == 0 and counts[2] > 1000, counts
        assert ((ras["tri"] >= 0) == (ras["hits"] == 2)).all()
        assert np.isfinite(ras["second"][ras["hits"] == 2]).all() and (ras["second"] >= ras["depth"]).all()
    rng = np.random.RandomState(5)
    for _ in range(50):
        a = rng.randint(2, 10, size=2)
        n = rng.randint(4, 20)
        c = a + n                                                       # the diagonal a -> c runs through n - 1 pixel centres
        b, d = a + [n + rng.randint(0, 6), -rng.randint(0, 4)], a + [-rng.randint(0, 4), n + rng.randint(0, 6)]
        q = [[int(v * 256 + 128) for v in p] for p in (a, b, c, d)]
        m1 = RC.coverage_mask([q[0][0], q[1][0], q[2][0]], [q[0][1], q[1][1], q[2][1]], 40, 40)
        m2 = RC.coverage_mask([q[0][0], q[2][0], q[3][0]], [q[0][1], q[2][1], q[3][1]], 40, 40)
        assert not (m1 & m2).any()
        on_diagonal = [(m1 | m2)[a[1] + k, a[0] + k] for k in range(1, n)]
        assert all(on_diagonal)
