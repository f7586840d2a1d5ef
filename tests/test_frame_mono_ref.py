"""tests/frame_mono_ref.py, the numpy restatement the device-built RGB-D / monocular Frame is held to, pinned on the CPU: the
pass-through rule, the residual of the five fixed iterations against the forward distortion model, and the crafted keypoints that must
fall outside the grid."""
import numpy as np

import frame_mono_ref as M

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def lattice(step=4):
    yy, xx = np.mgrid[0:M.H + 1:step, 0:M.W + 1:step]
    return np.stack([xx.ravel(), yy.ravel()], 1).astype(f32)


def test_zero_coefficients_give_the_input():
    xy = M.crafted_keypoints()["xy"]
    for dist in ((0, 0, 0, 0), (0, 0, 0, 0, 0)):
        assert np.array_equal(bits(M.undistort(xy, M.CAM, dist)), bits(xy))
    assert np.array_equal(M.image_bounds(M.W, M.H, M.CAM, (0, 0, 0, 0)), f32([0, M.W, 0, M.H]))


def test_k1_zero_passes_through_whatever_the_rest_holds():
    xy = M.crafted_keypoints()["xy"]
    dist = (0.0, -0.9, 0.01, 0.002, 1.1)
    assert np.array_equal(bits(M.undistort(xy, M.CAM, dist)), bits(xy))
    assert np.array_equal(bits(M.undistort(xy, M.CAM, dist[:4])), bits(xy))
    assert np.array_equal(M.image_bounds(M.W, M.H, M.CAM, dist), f32([0, M.W, 0, M.H]))
    # and a non-zero k1 does move the points
    assert np.abs(M.undistort(xy, M.CAM, M.DIST5) - xy).max() > 1.0


def test_round_trip_through_the_forward_model():
    xy = lattice(4)
    assert xy.shape[0] == 105 * 61
    un = M.undistort(xy, M.CAM, M.DIST5)
    err = np.linalg.norm(M.distort(un, M.CAM, M.DIST5) - xy.astype(np.float64), axis=1).max()
    print("round trip residual [px]", err)                                     # 0.0021 on this lattice, which includes the far borders x = 416 and y = 240
    assert err < 0.01
    # k3 matters on this camera: without it the result at the corners is another one
    with np.errstate(all="ignore"):
        assert np.abs(un - M.undistort(xy, M.CAM, M.DIST5[:4])).max() > 0.05


def test_crafted_keypoints_fall_outside_the_grid():
    b = M.image_bounds(M.W, M.H, M.CAM, M.DIST5)
    assert b[0] < 0 < M.W < b[1] or (b[1] - b[0]) != M.W                       # the bounds are the undistorted corners, not the image
    un = M.undistort(M.OUT_OF_GRID, M.CAM, M.DIST5)
    px, py, inside = M.grid_cell(un, b)
    assert px[0] == 64 and px[1] == 64 and py[2] == 48 and not inside.any()
    kp = M.crafted_keypoints()
    assert np.array_equal(kp["xy"][:3], M.OUT_OF_GRID) and kp["xy"].shape == (300, 2)
    _, _, ins = M.grid_cell(M.undistort(kp["xy"], M.CAM, M.DIST5), b)
    assert not ins[:3].any() and ins.sum() > 250


def test_depth_rules():
    xy = f32([[10.99, 7.999], [-0.5, -0.25], [-1.0, 3.0], [4.0, 3.0], [3.999, 2.0], [np.nan, 1.0], [1.0, np.inf], [2.0, 1.0], [0.0, 0.0], [1.0, 0.0], [3.0, 0]])
    d = np.arange(12 * 9, dtype=f32).reshape(9, 12) + 1
    d[1, 2] = np.nan; d[0, 1] = -2.0; d[0, 3] = np.inf
    small = d[:3, :4].copy()                                                   # 4 x 3: (4.0, 3.0) is outside, (3.999, 2.0) is its last pixel
    un = M.undistort(xy, M.CAM, M.DIST5)
    r = M.build(xy, M.CAM, M.DIST5, 40.0, d, 1.0)
    assert r["depth"][0] == d[7, 10] and r["depth"][1] == d[0, 0] and r["depth"][2] == -1 and r["depth"][5] == -1 and r["depth"][6] == -1
    assert bits(r["u_right"])[0] == bits(f32(un[0, 0] - f32(40.0) / d[7, 10]))
    r = M.build(xy, M.CAM, M.DIST5, 40.0, small, 1.0)
    assert r["depth"][3] == -1 and r["depth"][4] == small[2, 3] and r["depth"][0] == -1
    assert r["depth"][7] == -1 and r["u_right"][7] == -1                         # NaN
    assert r["depth"][9] == -1                                                   # negative
    assert np.isinf(r["depth"][10]) and bits(r["u_right"])[10] == bits(un[10, 0])   # +inf: mvuRight = u_un
    # the factor: untouched within 1e-5 of 1 on F32, always applied on U16
    a = M.build(xy, M.CAM, M.DIST5, 40.0, small, 1 + 5e-6); b = M.build(xy, M.CAM, M.DIST5, 40.0, small, 1.0)
    assert np.array_equal(bits(a["depth"]), bits(b["depth"]))
    h = M.build(xy, M.CAM, M.DIST5, 40.0, small, 0.5)
    assert h["depth"][4] == small[2, 3] * f32(0.5)
    u = np.full((3, 4), 5000, np.uint16); u[0, 0] = 0
    a = M.build(xy, M.CAM, M.DIST5, 40.0, u, 1 + 5e-6)
    assert bits(a["depth"])[4] == bits(f32(5000) * f32(1 + 5e-6)) and a["depth"][1] == -1 and a["depth"][4] != 5000
    m = M.build(xy, M.CAM, M.DIST5, 40.0, None)
    assert np.all(m["depth"] == -1) and np.all(m["u_right"] == -1) and np.array_equal(bits(m["xy_un"]), bits(un))
