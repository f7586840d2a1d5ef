"""Random calls of lld_orb_extract (ORBextractor::operator() on the device) against the CPU restatement tests/orb_extract_ref.py:
parameters over the whole accepted range with nudges toward its edges (1 or 16 levels, scale factors from just above 1 to 2.5,
0 or 1 feature up to 20000, thresholds from 1 to 255 in either order, patterns at the +-13 limit), 1-8 images per call of mixed
sizes from the validity boundary (a last level of 62 px) up to 1920x1080, mixed scene kinds, host, strided host and device input
with a step above the width.  Every keypoint field by its bit pattern, the descriptors (also through lld_orb_extractor_descriptors),
the per-level statistics and every pyramid level, bit for bit.  A third of the calls are repeated in reverse image order on the same
handle.  The restatement runs in a pool of worker processes that never open the GPU; the GPU is used from this process only.
      python tools/fuzz_orb_extract.py [n=1000] [seed=0] [workers=15]"""
import ctypes as C
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402

import orb_extract_ref as R  # noqa: E402
from orb_scenes import KINDS, scene  # noqa: E402

f32 = np.float32
MAX_COLS, MAX_ROWS = 1920, 1080
PIXEL_BUDGET = 6_000_000                  # level-0 pixels per call: keeps the restatement of one call within seconds
KIND_P = dict(textured=0.35, busy=0.2, flat=0.15, checker=0.1, corner=0.1, constant=0.1)


def min_side(inv_last):
    """Smallest level-0 side whose last level is >= 62 px (the smallest level with one FAST cell)."""
    c = max(62, int(61.0 / float(inv_last)) - 2)
    while R.level_size(c, c, inv_last)[0] < 62:
        c += 1
    return c


def draw_params(rng):
    u = rng.random()
    scale = f32(rng.choice([1.2, 1.2, 1.25, 1.5, 2.0, 1.05, 1.3])) if u < 0.5 else f32(rng.uniform(1.001, 2.5))
    n_levels = int(rng.choice([1, 2, 8, 16])) if rng.random() < 0.35 else int(rng.integers(1, 17))
    while n_levels > 1 and min_side(f32(1) / f32(scale ** (n_levels - 1))) > MAX_ROWS:
        n_levels -= 1                                      # the smallest valid image must fit 1920x1080
    u = rng.random()
    if u < 0.08: nfeatures = 0
    elif u < 0.16: nfeatures = 1
    elif u < 0.3: nfeatures = int(rng.choice([1000, 1200, 2000]))
    elif u < 0.38: nfeatures = int(rng.integers(5000, 20001))
    else: nfeatures = int(np.exp(rng.uniform(np.log(2), np.log(4000))))
    u = rng.random()
    if u < 0.2: ini, mn = 20, 7
    elif u < 0.3: ini, mn = 12, 7
    elif u < 0.4: ini = mn = int(rng.integers(1, 256))
    elif u < 0.5: ini = int(rng.integers(1, 255)); mn = int(rng.integers(ini + 1, 256))       # min > ini
    elif u < 0.55: ini = mn = 1
    elif u < 0.6: ini = mn = 255
    else: ini, mn = int(rng.integers(1, 256)), int(rng.integers(1, 256))
    return (nfeatures, float(scale), n_levels, ini, mn)


def draw_size(rng, T):
    inv_last = T["inv_scale"][-1]
    lo = min_side(inv_last)
    for _ in range(100):
        u = rng.random()
        if u < 0.15:                                           # at the boundary, or a few pixels above it
            c, r = lo + int(rng.integers(0, 4)), lo + int(rng.integers(0, 4))
        elif u < 0.3:
            c, r = int(rng.integers(1280, MAX_COLS + 1)), int(rng.integers(720, MAX_ROWS + 1))
        elif u < 0.4:                                          # panorama: many initial octree nodes
            r = lo + int(rng.integers(0, 40)); c = int(rng.integers(4 * r, 16 * r + 1))
        else:
            c = int(np.exp(rng.uniform(np.log(lo), np.log(MAX_COLS)))); r = int(np.exp(rng.uniform(np.log(lo), np.log(MAX_ROWS))))
        c, r = min(max(c, lo), MAX_COLS), min(max(r, lo), MAX_ROWS)
        if R.image_ok(c, r, T):
            return c, r
    return lo, lo


def draw(rng):
    """One call: dict(params, pattern_seed, pattern_kind, images [dict(kind, cols, rows, seed, mode, pad)], max_cols, max_rows,
    max_images, repeat)."""
    params = draw_params(rng)
    T = R.level_tables(*params[:3])
    n = int(rng.integers(1, 9))
    images, area = [], 0
    kinds = list(KIND_P); p = np.array([KIND_P[k] for k in kinds])
    for _ in range(n):
        c, r = draw_size(rng, T)
        if area + c * r > PIXEL_BUDGET:
            lo = min_side(T["inv_scale"][-1]); c, r = lo + int(rng.integers(0, 60)), lo + int(rng.integers(0, 30))
            c, r = min(c, MAX_COLS), min(r, MAX_ROWS)
            if not R.image_ok(c, r, T):
                c = r = lo
        area += c * r
        mode = str(rng.choice(["host", "host", "strided", "device"]))
        pad = int(rng.choice([1, 3, 64, 256 - c % 256 if c % 256 else 256])) if mode != "host" else 0
        images.append(dict(kind=str(rng.choice(kinds, p=p)), cols=c, rows=r, seed=int(rng.integers(0, 1 << 30)), mode=mode, pad=pad))
    mc, mr = max(im["cols"] for im in images), max(im["rows"] for im in images)
    if rng.random() < 0.3:
        mc, mr = min(MAX_COLS, mc + int(rng.integers(0, 300))), min(MAX_ROWS, mr + int(rng.integers(0, 200)))
    mi = n if rng.random() < 0.6 else int(rng.integers(n, 9))
    return dict(params=params, pattern_seed=int(rng.integers(0, 1 << 30)), pattern_kind=str(rng.choice(["seeded", "seeded", "edge"])),
                images=images, max_cols=mc, max_rows=mr, max_images=mi, repeat=bool(rng.random() < 0.33))


def pattern(case):
    """[256][4] pattern coordinates in [-13, 13]; 'edge' puts every coordinate at +-13 (descriptor reads up to 18 px away)."""
    g = np.random.default_rng(case["pattern_seed"])
    if case["pattern_kind"] == "edge":
        return (13 * g.choice([-1, 1], size=(256, 4))).astype(np.int32)
    return g.integers(-13, 14, size=(256, 4)).astype(np.int32)


def image(im):
    return scene(im["kind"], im["cols"], im["rows"], im["seed"])


def expected(case):
    """The restatement's result for every image of the call (no GPU): keypoints, descriptors, statistics and pyramid."""
    pat = pattern(case)
    out = []
    for im in case["images"]:
        e = R.extract(image(im), *case["params"], pat)
        e.pop("candidates"); e.pop("tables")
        out.append(e)
    return out


# ------------------------------------------------------------------------------------------------------------- device side
def download(ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return out


def differences(ex, got, exp, index):
    """Names of the outputs of image `index` that differ from the restatement (empty: bit for bit equal)."""
    from lld_slam_amd import vocabulary as voc
    bad = []
    for f in ("xy", "octave", "angle", "response", "size", "desc"):
        g, e = np.asarray(got[f]), exp[f]
        if g.shape != e.shape or not np.array_equal(g.view(np.uint32) if g.dtype.kind == "f" else g, e.view(np.uint32) if e.dtype.kind == "f" else e):
            bad.append(f)
    if not np.array_equal(got["stats"], exp["stats"]):
        bad.append("stats")
    lv, cols, rows, step = ex.pyramid(index)
    for l, lev in enumerate(exp["levels"]):
        if (rows[l], cols[l]) != lev.shape or step[l] != cols[l] or not np.array_equal(
                download(C.cast(lv[l], C.c_void_p).value, int(rows[l]) * int(step[l])).reshape(rows[l], step[l]), lev):
            bad.append(f"level{l}")
    ptr, n = voc.extractor_descriptors(ex, index)
    if n != len(exp["desc"]) or (n and not np.array_equal(download(ptr, n * 32).view(np.uint32).reshape(n, 8), exp["desc"])):
        bad.append("device_desc")
    return bad


def inputs(case, keep):
    """The call's lld_orb_image inputs: contiguous host arrays, host views of a wider array (step = strides[0]) or device copies
    with step = cols + pad."""
    out = []
    for im in case["images"]:
        img = image(im)
        if im["mode"] == "strided":
            big = np.zeros((im["rows"], im["cols"] + im["pad"]), np.uint8); big[:, :im["cols"]] = img
            out.append(big[:, :im["cols"]]); keep.append(big)
        elif im["mode"] == "device":
            import torch
            t = torch.zeros((im["rows"], im["cols"] + im["pad"]), dtype=torch.uint8, device="cuda:0")
            t[:, :im["cols"]] = torch.from_numpy(img).to("cuda:0")
            torch.cuda.synchronize()
            keep.append(t)
            out.append((t.data_ptr(), im["cols"], im["rows"], im["cols"] + im["pad"]))
        else:
            out.append(img)
    return out


def run_case(ctx, case, exp):
    """Device call(s) of one case against `exp`.  Returns (list of differences as 'image:output', keypoints)."""
    from lld_slam_amd import abi
    from lld_slam_amd.orb_extractor import ORBextractor
    keep = []
    ims = inputs(case, keep)
    bad = []
    with ORBextractor(ctx, *case["params"], pattern(case), max_cols=case["max_cols"], max_rows=case["max_rows"],
                      max_images=case["max_images"]) as ex:
        orders = [list(range(len(ims)))] + ([list(range(len(ims)))[::-1]] if case["repeat"] else [])
        for order in orders:
            st, res = ex.extract_raw([ims[i] for i in order])
            if st != abi.LLD_OK:
                return [f"status {st}"], 0
            for k, i in enumerate(order):
                bad += [f"{i}:{f}" for f in differences(ex, res[k], exp[i], k)]
    return bad, sum(len(e["octave"]) for e in exp)


def r_extract(ctx, rng, sid):
    """One drawn call (the restatement in this process): (bit for bit equal, keypoints)."""
    case = draw(rng)
    bad, nk = run_case(ctx, case, expected(case))
    return not bad, nk


ROUTINES = dict(extract=r_extract)


def describe(case):
    p = case["params"]
    ims = " ".join(f"{im['kind'][:4]}{im['cols']}x{im['rows']}{'' if im['mode'] == 'host' else im['mode'][0] + str(im['pad'])}" for im in case["images"])
    return f"N={p[0]} s={p[1]:.4f} L={p[2]} th={p[3]}/{p[4]} pat={case['pattern_kind']} max={case['max_cols']}x{case['max_rows']}x{case['max_images']}{' rep' if case['repeat'] else ''} [{ims}]"


def _expected_job(arg):
    it, case = arg
    t0 = time.time()
    try:
        return it, expected(case), None, time.time() - t0
    except Exception as e:                                       # the restatement refusing a drawn call is a finding too
        return it, None, f"{type(e).__name__}: {e}", time.time() - t0


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    workers = min(int(sys.argv[3]) if len(sys.argv) > 3 else 15, 16)
    cases = [(it, draw(np.random.default_rng([seed, it]))) for it in range(n)]
    t_all = time.time()
    print(f"# tools/fuzz_orb_extract.py {n} {seed} {workers}: random lld_orb_extract calls, device vs tests/orb_extract_ref.py, "
          f"every output bit for bit", flush=True)
    pool = mp.get_context("spawn").Pool(workers)                # started before this process opens the GPU; the workers never do
    from lld_slam_amd import Context
    ctx = Context(0)
    tot = dict(cases=0, diff=0, images=0, keypoints=0, cpu_s=0.0, gpu_s=0.0)
    levels_hit = dict(n1=0, n16=0, nf0=0, th255=0, empty_level=0, sorted=0, wide=0)
    for it, exp, err, cpu_s in pool.imap(_expected_job, cases):
        case = cases[it][1]
        t0 = time.time()
        if err is None:
            try:
                bad, nk = run_case(ctx, case, exp)
            except Exception as e:
                bad, nk = [f"{type(e).__name__}: {e}"], 0
        else:
            bad, nk = [f"restatement {err}"], 0
        gpu_s = time.time() - t0
        tot["cases"] += 1; tot["diff"] += bool(bad); tot["images"] += len(case["images"]); tot["keypoints"] += nk
        tot["cpu_s"] += cpu_s; tot["gpu_s"] += gpu_s
        if exp:
            S = np.concatenate([e["stats"] for e in exp])
            levels_hit["n1"] += case["params"][2] == 1; levels_hit["n16"] += case["params"][2] == 16
            levels_hit["nf0"] += case["params"][0] == 0; levels_hit["th255"] += case["params"][3:] == (255, 255)
            levels_hit["empty_level"] += int((S[:, 0] == 0).any()); levels_hit["sorted"] += int((S[:, 4] > 0).any())
            levels_hit["wide"] += int((S[:, 6] > S[:, 7] + 3).any())
        print(f"{'DIFF' if bad else 'ok  '} it={it:<5} kp={nk:<7} cpu={cpu_s:6.2f}s gpu={gpu_s:5.2f}s {describe(case)}"
              + (f"  differs: {' '.join(bad[:12])}" if bad else ""), flush=True)
    pool.close(); pool.join()
    ctx.close()
    print(f"# cases {tot['cases']}  differences {tot['diff']}  images {tot['images']}  keypoints {tot['keypoints']}  "
          f"restatement {tot['cpu_s']:.0f} s (in {workers} workers)  device side {tot['gpu_s']:.0f} s  wall {time.time() - t_all:.0f} s")
    print("# calls with: " + "  ".join(f"{k} {v}" for k, v in levels_hit.items()))
    return 1 if tot["diff"] else 0


if __name__ == "__main__":
    sys.exit(main())
