"""GPU parity of Optimizer::OptimizeEssentialGraph on graphs shaped like the reference's (tests/posegraph_scenes.py): fill tiles,
rows with more than sixteen K tiles, multi-workgroup back substitution, edges with edge_i < edge_j, fixed vertices in the middle,
every padding of the last tile, awkward structures and the dense / PCG size boundary.  Held to test_gpu_posegraph's bars."""
import dataclasses
import functools

import numpy as np
import pytest

import posegraph_scenes as S
from lld_slam_amd import Context, Optimizer
from test_gpu_posegraph import _check, deviation

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _oracle_pair(key, fix, iterations=15):
    """(oracle, FMA twin) for a graph built by `_GRAPHS[key]` - cached: both solvers are held to the same oracle run."""
    import oracle_py
    gr = _GRAPHS[key]()
    return (oracle_py.optimize_essential_graph(gr, bFixScale=fix, iterations=iterations),
            oracle_py.optimize_essential_graph(gr, bFixScale=fix, iterations=iterations, fma=True))


def _against_oracle(gpu_ctx, key, fix, solver, **kw):
    gr = _GRAPHS[key]()
    g = Optimizer(gpu_ctx).OptimizeEssentialGraph(gr, bFixScale=fix, solver=solver, **kw)
    o, twin = _oracle_pair(key, fix, **kw)
    _check(g, o, deviation(twin, o))
    fixed = np.asarray(gr.fixed).astype(bool)
    np.testing.assert_array_equal(g.sim3[fixed], gr.sim3[fixed])     # fixed vertices are not touched
    return g, o


def _with(gr, keep=None, add=()):
    """gr with only the edges `keep` (boolean mask) plus `add` = [(i, j, Sji)]."""
    keep = np.ones(len(gr.edge_i), bool) if keep is None else keep
    ei = np.concatenate([gr.edge_i[keep], np.array([a[0] for a in add], np.int32)]).astype(np.int32)
    ej = np.concatenate([gr.edge_j[keep], np.array([a[1] for a in add], np.int32)]).astype(np.int32)
    sji = np.vstack([gr.edge_sji[keep]] + [np.asarray(a[2])[None] for a in add])
    return dataclasses.replace(gr, edge_i=ei, edge_j=ej, edge_sji=sji)


def _meas(gr, i, j, src="sim3"):
    return S._from_mat(S._mat(gr.sim3[j] if src == "sim3" else gr.meta["gt"][j]) @ np.linalg.inv(S._mat(gr.sim3[i] if src == "sim3" else gr.meta["gt"][i])))


def _isolated():
    """keyframe 10 of a small scene has no edge at all (a free vertex with a zero block: lambda I alone)"""
    gr = S.make_loop_scene(seed=11, n_kf=40, loop_kf=28, cur_conn=3, loop_conn=4, earlier_loops=1)
    return _with(gr, keep=(gr.edge_i != 10) & (gr.edge_j != 10))


def _fixed_only():
    """keyframe 20 is linked only to fixed keyframes (28 = pLoopKF and 5): its row of H has no off-diagonal block"""
    gr = S.make_loop_scene(seed=12, n_kf=40, loop_kf=28, cur_conn=3, loop_conn=4, earlier_loops=1, extra_fixed=(5,))
    keep = (gr.edge_i != 20) & (gr.edge_j != 20)
    return _with(gr, keep=keep, add=[(20, 28, _meas(gr, 20, 28, "gt")), (5, 20, _meas(gr, 5, 20, "gt"))])


def _double_edges():
    """the same pair joined twice: a second loop edge beside the first (other measurement), a covisibility edge repeated the
    other way round"""
    gr = S.make_loop_scene(seed=13, n_kf=40, loop_kf=28, cur_conn=3, loop_conn=4, earlier_loops=1)
    return _with(gr, add=[(39, 27, _meas(gr, 39, 27, "gt")), (12, 14, _meas(gr, 12, 14))])


_GRAPHS = {("scene", n): (lambda n=n: S.scene(n)[0]) for n in S.SCENES}
_GRAPHS.update({("pad", nu): (lambda nu=nu: S.make_padding_graph(nu)) for nu in S.PADDING_SIZES})
_GRAPHS.update({("reversed", n): (lambda n=n: S.reverse_edges(S.scene(n)[0], seed=5)[0]) for n in ("reparented", "short_free")})
_GRAPHS.update({("odd", "isolated"): _isolated, ("odd", "fixed_only"): _fixed_only, ("odd", "double_edges"): _double_edges})


@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("name", list(S.SCENES))
def test_scene_matches_oracle(gpu_ctx, name, solver):
    g, o = _against_oracle(gpu_ctx, ("scene", name), S.SCENES[name][1], solver)
    assert g.solver_used == solver and (g.pcg_iterations > 0) == (solver == 2)


WELL_CONDITIONED = ["mid_loop", "many_to_many", "reparented", "fixed_many"]          # fixed scale: no flat valley


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("name", WELL_CONDITIONED)
def test_scene_at_equal_iteration_counts(gpu_ctx, name, k):
    """As test_essential_graph_at_equal_iteration_counts: the same k iterations on both sides, the plain 1e-5 bar on every pose."""
    g, o = _against_oracle(gpu_ctx, ("scene", name), True, 0, iterations=k)
    assert g.lm_iterations == o.lm_iterations and g.solver_used == 1
    assert (deviation(g, o)[:3] <= 1e-5).all(), deviation(g, o)


@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("nu", S.PADDING_SIZES)
def test_padding_sweep(gpu_ctx, nu, solver):
    """7 nu mod 16 through every residue: the identity rows that pad the last tile, and the right-hand side row behind them."""
    _against_oracle(gpu_ctx, ("pad", nu), True, solver)


@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("name", ["reparented", "short_free"])
def test_reversed_edges(gpu_ctx, name, solver):
    """Half of the edges written (j, i, Sji^-1): the hi < hj side of the dense fill and of the PCG matvec."""
    _against_oracle(gpu_ctx, ("reversed", name), S.SCENES[name][1], solver)


@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("kind", ["isolated", "fixed_only", "double_edges"])
def test_awkward_structures(gpu_ctx, kind, solver):
    g, o = _against_oracle(gpu_ctx, ("odd", kind), True, solver)
    if kind == "isolated":
        np.testing.assert_array_equal(g.sim3[10], _GRAPHS[("odd", kind)]().sim3[10])


def test_self_edges_are_refused(gpu_ctx):
    gr = S.scene("short_free")[0]
    for e in (0, len(gr.edge_i) - 1):                          # a LoopConnection (free - free) and a covisibility edge
        ej = gr.edge_j.copy(); ej[e] = gr.edge_i[e]
        for solver in (0, 1, 2):
            with pytest.raises(RuntimeError):
                Optimizer(gpu_ctx).OptimizeEssentialGraph(dataclasses.replace(gr, edge_j=ej), solver=solver)
    lk = int(gr.meta["loop_kf"])                               # a self-edge on the fixed vertex too
    g2 = _with(gr, add=[(lk, lk, np.array([0, 0, 0, 1, 0, 0, 0, 1.0]))])
    with pytest.raises(RuntimeError):
        Optimizer(gpu_ctx).OptimizeEssentialGraph(g2)


def _chain_with_loops(n_kf, loops=8):
    """n_kf keyframes, keyframe 0 fixed: a chain with covisibility 3 and `loops` loop edges between free keyframes, plus a few onto
    keyframe 0, so that the PCG converges in a few thousand iterations."""
    gr = S.make_loop_scene(seed=20, n_kf=n_kf, laps=4, loop_kf=0, cur_conn=1, loop_conn=1, n_corrected=1, earlier_loops=loops,
                           drift=(0.0005, 0.005))
    anchors = [(k, 0, _meas(gr, k, 0, "gt")) for k in range(n_kf // 8, n_kf, n_kf // 8)]
    return _with(gr, add=anchors)


def test_dense_pcg_size_boundary():
    """nu = 4681 (NT = 2048) is the largest system the dense path takes by default; nu = 4682 (NT = 2049) goes to the PCG and
    solver = 1 is refused.  The oracle's dense LDL^T at this size would take hours: the dense result is held to the PCG's, as
    test_essential_graph_default_solver_is_dense_and_agrees_with_pcg does.  Its own context: the 8.6 GB of dense scratch stay with
    a context until it is destroyed."""
    with Context(0) as ctx:
        opt = Optimizer(ctx)
        gr = _chain_with_loops(4682)
        assert int((gr.fixed == 0).sum()) == 4681 and (7 * 4681 + 15) // 16 == 2048
        d = opt.OptimizeEssentialGraph(gr, iterations=1)
        p = opt.OptimizeEssentialGraph(gr, iterations=1, solver=2)
        assert d.solver_used == 1 and p.solver_used == 2 and d.lm_iterations == p.lm_iterations == 1
        assert (deviation(d, p) <= [1e-5, 1e-5, 1e-5, 1e-4]).all(), deviation(d, p)
        assert np.abs(d.sim3 - gr.sim3).max() > 1e-4                 # the step did something
        big = _chain_with_loops(4683)
        assert (7 * int((big.fixed == 0).sum()) + 15) // 16 == 2049
        with pytest.raises(RuntimeError):
            opt.OptimizeEssentialGraph(big, iterations=1, solver=1)
        q = opt.OptimizeEssentialGraph(big, iterations=1)
        assert q.solver_used == 2 and q.pcg_iterations > 0 and np.isfinite(q.sim3).all()
