"""Secondary measurements (not the driver's bench line): every operator of the
path at ~10 M dofs on one MI355X -- BASELINE.json configs[1] (P4 stiffness) and
configs[2] (P6 mass, lumped and dense/TSMM form) plus neighbours.  Prints one
JSON object per line; HIP-event medians, inputs resident in HBM."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import wave_fenics_amd as w  # noqa: E402
from wave_fenics_amd import la  # noqa: E402
from wave_fenics_amd._lib import WF_FLAG_ORDERED  # noqa: E402


def timeit(fn, reps=20, warm=3, settle_s=0.4):
    """HIP-event median of `reps` calls at the GPU's sustained operating point: after `warm` calls the
    function is run untimed for `settle_s` seconds, because the first ~60 launches after idle run up to 25 %
    slower while board power ramps (profiles/r03_power_ramp.md).  SETTLE=0 in the environment times from idle."""
    import time
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    settle_s = float(os.environ.get("SETTLE", settle_s))
    t0 = time.time()
    while time.time() - t0 < settle_s:
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def report(name, ms, alg_bytes, ndofs, extra=None):
    out = {"op": name, "ms": round(ms, 4), "alg_GBs": round(alg_bytes / ms / 1e6, 1),
           "frac_of_8TBs": round(alg_bytes / ms / 1e6 / 8000, 3), "Gdofs_per_s": round(ndofs / ms / 1e6, 2)}
    if extra:
        out.update(extra)
    print(json.dumps(out), flush=True)


def gl_rule(m):
    x, wt = np.polynomial.legendre.leggauss(m)
    return 0.5 * (x + 1), 0.5 * wt


def lagrange(nodes, pts):
    n = len(nodes)
    phi = np.ones((len(pts), n))
    for a in range(n):
        for b in range(n):
            if b != a:
                phi[:, a] *= (pts - nodes[b]) / (nodes[a] - nodes[b])
    return phi


def gll_rule(m):
    """m-point Gauss-Lobatto-Legendre rule on [0, 1] (the GLL rule of degree 2 m - 3, which tabulate_gll gives with the
    nodes of degree m - 1)."""
    pts, wts, _ = w.tabulate_gll(m - 1)
    return pts, wts


def bench_dense_rect(V, mesh, p, x, y, tag):
    """Dense mass with a rectangular table: Gauss with P+2 points and the GLL rule of degree P+1 where it is not square
    (4, 5, 5, 6 points at P4..P7), each on the default any-rule kernel and on the marching kernel asked for with
    {"kernel": "mass_march"}.  The two operators are timed alternately, RECT_ROUNDS times (default 3): the median and the
    spread of the rounds.  A pair the marching kernel is not compiled for prints its default line only."""
    N, n = V.ndofs, p + 1
    rules = [("gauss", gl_rule(p + 2), np.linspace(0, 1, n))]
    mg = max(2, (p + 5) // 2)
    if mg != n:
        rules.append(("gll", gll_rule(mg), w.tabulate_gll(p)[0]))
    rounds = int(os.environ.get("RECT_ROUNDS", "3"))
    for label, (qp, qw), nodes in rules:
        phi1, m = lagrange(nodes, qp), len(qp)
        W3 = np.einsum("k,j,i->kji", qw, qw, qw).reshape(-1)
        detq = np.tile(W3 / mesh.ncells, (mesh.ncells, 1))     # affine box: detJ = vol * w_q
        ops = [("default", w.MassOperator(V, p, phi1, detq))]
        try:
            ops.append(("mass_march", w.MassOperator(V, p, phi1, detq, tuning={"kernel": "mass_march"})))
        except w.WavehipError:
            pass
        del detq
        ms = {name: [] for name, _ in ops}
        for _ in range(rounds):
            for name, op in ops:
                ms[name].append(timeit(lambda: op.apply(x, y), reps=10))
        for name, op in ops:
            t = float(np.median(ms[name]))
            report(f"dense mass P{p} {label} {m} points [{name}]", t, op.alg_bytes(), N,
                   dict(tag, nq1=m, kernel=op.kernel, alg_bytes=op.alg_bytes(), ms_rounds=[round(v, 4) for v in ms[name]],
                        ns_per_detJ_KB=round(t * 1e6 / (8.0 * mesh.ncells * m ** 3 / 1024), 4), lz=op.info.plan_lz))
        del ops


def bench_tet(dev):
    import time
    from wave_fenics_amd import tet
    p, n = 4, int(os.environ.get("TET_N", "54"))
    t0 = time.time()
    V = tet.create_kuhn_box(n, p)
    t1 = time.time()
    op = tet.TetStiffnessOperator(V, p)
    t2 = time.time()
    mass = tet.TetMassOperator(V, p)           # rule of degree 2p = 8: 125 points
    t3 = time.time()
    N = V.ndofs
    x = torch.rand(N, dtype=torch.float64, device=dev)
    y = torch.zeros(N, dtype=torch.float64, device=dev)
    # the two operators alternately, TET_ROUNDS times (default 5): the median and the spread of the rounds
    rounds = int(os.environ.get("TET_ROUNDS", "5"))
    ms_k, ms_m = [], []
    for _ in range(rounds):
        ms_k.append(timeit(lambda: op(x, y)))
        ms_m.append(timeit(lambda: mass(x, y)))
    ms = float(np.median(ms_k))
    report(f"tet P{p} dense stiffness (MFMA f64 16x16x4), Kuhn box {n}^3 cubes", ms, op.alg_bytes(), N,
           {"cells": V.ncells, "ndofs": N, "TFLOPs_dense_model": round(op.flops() / ms / 1e9, 2),
            "frac_of_f64_mfma_peak_78.6TF": round(op.flops() / ms / 1e9 / 78.6, 3),
            "ms_rounds": [round(v, 4) for v in ms_k], "mesh_s": round(t1 - t0, 2), "setup_s": round(t2 - t1, 2)})
    ms = float(np.median(ms_m))
    report(f"tet P{p} dense mass (MFMA f64 16x16x4, A = Phi^T W Phi), Kuhn box {n}^3 cubes, {mass.num_quads()}-point rule", ms,
           mass.alg_bytes(), N,
           {"cells": V.ncells, "ndofs": N, "kernel": mass.kernel, "alg_bytes": mass.alg_bytes(),
            "ms_rounds": [round(v, 4) for v in ms_m], "ms_over_stiffness": round(ms / float(np.median(ms_k)), 3),
            "setup_s": round(t3 - t2, 2)})


def bench_medium(dev):
    """Cell coefficients: the P4 box apply (owner kernel) and the P4 tetrahedral stiffness apply at ~10.2 M dofs, each with
    and without a coefficient array, alternating in one process (MEDIUM_ROUNDS rounds, default 7; every timing after the
    settle protocol of timeit).  A box coefficient is folded into the stored geometry: same kernel, same bytes.  The
    tetrahedral stiffness runs its coefficient variant (one more double per cell)."""
    from wave_fenics_amd import tet
    rounds = int(os.environ.get("MEDIUM_ROUNDS", "7"))
    p = 4

    def alternate(plain, coeff, x, y):
        ms = {"plain": [], "coeff": []}
        for _ in range(rounds):
            ms["plain"].append(timeit(lambda: plain(x, y)))
            ms["coeff"].append(timeit(lambda: coeff(x, y)))
        return ms

    def lines(name, ops, ms, N, extra):
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k in ("plain", "coeff"):
            op = ops[k]
            report(f"{name} [{op.kernel}] " + ("with cell_coeff" if k == "coeff" else "without"), med[k], op.alg_bytes(), N,
                   dict(extra, cell_coeff=op.cell_coeff, kernel=op.kernel, geometry=op.geometry, metric=op.metric, update=op.update,
                        lz=op.info.plan_lz, alg_bytes=op.alg_bytes(), device_bytes=op.info.device_bytes,
                        ms_rounds=[round(v, 4) for v in ms[k]], spread=round((max(ms[k]) - min(ms[k])) / med[k], 4),
                        coeff_over_plain=round(med["coeff"] / med["plain"], 4)))

    if "MEDIUM_SKIP_BOX" not in os.environ:
        n = 54
        mesh = w.create_box(n, hi=(float(n),) * 3)     # unit cubes: affine by the bitwise rule, the owner form
        V = w.create_functionspace(mesh, p, build_dofmap=False)
        a = 0.5 + np.modf(1.618033988749895 * np.arange(mesh.ncells))[0] * 3.5
        ops = {"plain": w.StiffnessOperator(V, p), "coeff": w.StiffnessOperator(V, p, cell_coeff=a)}
        N = V.ndofs
        x = torch.rand(N, dtype=torch.float64, device=dev)
        y = torch.zeros(N, dtype=torch.float64, device=dev)
        lines(f"stiffness P{p} box {n}^3", ops, alternate(ops["plain"], ops["coeff"], x, y), N,
              {"degree": p, "cells": mesh.ncells, "ndofs": N, "runs": [len(ops[k].runs()) for k in ("plain", "coeff")]})
        del ops, x, y, V, mesh
        torch.cuda.empty_cache()
    n = int(os.environ.get("TET_N", "54"))
    V = tet.create_kuhn_box(n, p)
    a = 0.5 + np.modf(1.618033988749895 * np.arange(V.ncells))[0] * 3.5
    ops = {"plain": tet.TetStiffnessOperator(V, p), "coeff": tet.TetStiffnessOperator(V, p, cell_coeff=a)}
    N = V.ndofs
    x = torch.rand(N, dtype=torch.float64, device=dev)
    y = torch.zeros(N, dtype=torch.float64, device=dev)
    lines(f"tet P{p} dense stiffness, Kuhn box {n}^3 cubes", ops, alternate(ops["plain"], ops["coeff"], x, y), N,
          {"cells": V.ncells, "ndofs": N})


def bench_cellform(dev):
    """Cell forms on the cfg2 box (P4, 54^3 cells, ~10.2 M dofs) next to the applies that read the same data, alternating
    in one process (CELLFORM_ROUNDS rounds, default 5; every timing after the settle protocol of timeit):
      (a) the default stiffness apply;  (b) the apply under tuning = {"kernel": "elementwise"}, per-point geometry -- the
      kernel whose body the per-point form shares, and its yardstick;  (c) the per-point form;  (d) the per-cell form;
      (e) the lumped form.  One line per leg: median and range of the rounds."""
    rounds = int(os.environ.get("CELLFORM_ROUNDS", "5"))
    p, n = 4, int(os.environ.get("CELLFORM_N", "54"))
    mesh = w.create_box(n)
    V = w.create_functionspace(mesh, p, build_dofmap=True)
    N = V.ndofs
    x = torch.rand(N, dtype=torch.float64, device=dev)
    lam = torch.rand(N, dtype=torch.float64, device=dev)
    y = torch.zeros(N, dtype=torch.float64, device=dev)
    out = torch.zeros(mesh.ncells, dtype=torch.float64, device=dev)
    apply_default = w.StiffnessOperator(V, p)
    apply_elementwise = w.StiffnessOperator(V, p, structured=False, tuning={"kernel": "elementwise", "keep_cell_order": True})
    form_point = w.CellForm(V, p, tuning={"geometry": "per_point"})
    form_cell = w.CellForm(V, p)
    form_lumped = w.CellForm(V, p, "mass_lumped")
    assert (apply_elementwise.kernel, form_point.geometry, form_cell.geometry) == ("elementwise", "per_point", "per_cell")
    legs = [("a", f"stiffness apply [{apply_default.kernel} {apply_default.update}]", lambda: apply_default(x, y), apply_default.alg_bytes(),
             apply_default.info.device_bytes),
            ("b", "stiffness apply [elementwise, per point]", lambda: apply_elementwise(x, y), apply_elementwise.alg_bytes(),
             apply_elementwise.info.device_bytes),
            ("c", "cell form stiffness [per point]", lambda: form_point.eval(lam, x, out=out), form_point.info.alg_bytes,
             form_point.info.device_bytes),
            ("d", "cell form stiffness [per cell]", lambda: form_cell.eval(lam, x, out=out), form_cell.info.alg_bytes,
             form_cell.info.device_bytes),
            ("e", "cell form lumped mass", lambda: form_lumped.eval(lam, x, out=out), form_lumped.info.alg_bytes,
             form_lumped.info.device_bytes)]
    ms = {leg[0]: [] for leg in legs}
    for _ in range(rounds):
        for key, _, fn, _, _ in legs:
            ms[key].append(timeit(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for key, name, _, alg_bytes, device_bytes in legs:
        report(f"({key}) {name} P{p} box {n}^3", med[key], alg_bytes, N,
               {"cells": mesh.ncells, "ndofs": N, "alg_bytes": alg_bytes, "device_bytes": device_bytes,
                "ms_rounds": [round(v, 4) for v in ms[key]], "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4),
                "over_b": round(med[key] / med["b"], 4)})


def bench_tet_against(dev, other_path):
    """The default (no coefficient) P4 tetrahedral stiffness apply and mass apply of this library against ANOTHER build of
    libwavehip -- the parent commit's, say -- with both libraries loaded into this one process, the same operator created
    through each and the applies alternating (MEDIUM_ROUNDS rounds, default 7), first for the stiffness, then for the
    mass.  `python tools/bench_ops.py tet-ab` with the other library's path in WAVEHIP_LIB_B.  Only
    wf_op_create_dense_simplex, wf_op_create_dense_simplex_mass, wf_op_apply and wf_op_destroy of the other library are
    called, with this tree's descriptors: an older library reads the leading fields it knows."""
    import ctypes
    from wave_fenics_amd import _lib, tet
    from wave_fenics_amd.operators import _dp, _ip
    libs = {"this library": w.lib(), "other library": ctypes.CDLL(other_path)}
    other = libs["other library"]
    for create, desc in (("wf_op_create_dense_simplex", _lib.DenseDesc), ("wf_op_create_dense_simplex_mass", _lib.DenseMassDesc)):
        getattr(other, create).restype = ctypes.c_int
        getattr(other, create).argtypes = [ctypes.POINTER(desc), ctypes.POINTER(ctypes.c_void_p)]
    other.wf_op_apply.restype = ctypes.c_int
    other.wf_op_apply.argtypes = [ctypes.c_void_p] * 4
    other.wf_op_destroy.argtypes = [ctypes.c_void_p]
    p, n = 4, int(os.environ.get("TET_N", "54"))
    V = tet.create_kuhn_box(n, p)
    dm, xv, gd = (np.ascontiguousarray(V.dofmap, dtype=np.int32), np.ascontiguousarray(V.x, dtype=np.float64),
                  np.ascontiguousarray(V.geom_dofmap, dtype=np.int32))
    N = V.ndofs
    x = torch.rand(N, dtype=torch.float64, device=dev)
    y = torch.zeros(N, dtype=torch.float64, device=dev)

    def mesh_fields(d, nd, nq):
        d.nd, d.nq, d.ncells, d.ndofs = nd, nq, V.ncells, V.ndofs
        d.h_dofmap, d.nverts, d.h_xverts, d.h_geom_dofmap = _ip(dm), xv.shape[0], _dp(xv), _ip(gd)
        d.flags = 0

    def alternate(what, create, d):
        handles = {}
        for name, L in libs.items():
            handles[name] = ctypes.c_void_p()
            rc = getattr(L, create)(ctypes.byref(d), ctypes.byref(handles[name]))
            if rc != 0:
                raise RuntimeError(f"{name}: {create} returned {rc}")
        once = {}
        for name, L in libs.items():
            y.zero_()
            L.wf_op_apply(handles[name], x.data_ptr(), y.data_ptr(), 0)
            torch.cuda.synchronize()
            once[name] = y.clone()
        ms = {name: [] for name in libs}
        for _ in range(int(os.environ.get("MEDIUM_ROUNDS", "7"))):
            for name in ("other library", "this library"):
                ms[name].append(timeit(lambda: libs[name].wf_op_apply(handles[name], x.data_ptr(), y.data_ptr(), 0)))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for name in libs:
            print(json.dumps({"op": f"tet P{p} dense {what} without a coefficient, Kuhn box {n}^3 cubes, {name}", "ms": round(med[name], 4),
                              "ms_rounds": [round(v, 4) for v in ms[name]], "cells": V.ncells, "ndofs": N,
                              "this_over_other": round(med["this library"] / med["other library"], 4),
                              "max_abs_diff_of_one_apply": float((once["this library"] - once["other library"]).abs().max()),
                              "max_abs_y": float(once["this library"].abs().max())}), flush=True)
        for name, L in libs.items():
            L.wf_op_destroy(handles[name])

    X, W = tet.tet_quadrature(p)                  # the rule of tet.TetStiffnessOperator: degree 2p - 2, m = p
    dphi = np.ascontiguousarray(tet.clamp101(tet.tabulate_tet(p, X)[1]))
    W = np.ascontiguousarray(W)
    d = _lib.DenseDesc()
    mesh_fields(d, dphi.shape[2], dphi.shape[1])
    d.h_dphi, d.h_weights, d.c0 = _dp(dphi), _dp(W), 1500.0
    alternate("stiffness", "wf_op_create_dense_simplex", d)
    X, W = tet.tet_quadrature(p + 1)              # the rule of tet.TetMassOperator: degree 2p, 125 points
    phi = np.ascontiguousarray(tet.tabulate_tet(p, X)[0], dtype=np.float64)
    W = np.ascontiguousarray(W)
    d = _lib.DenseMassDesc()
    mesh_fields(d, phi.shape[1], phi.shape[0])
    d.h_phi, d.h_weights = _dp(phi), _dp(W)
    alternate("mass", "wf_op_create_dense_simplex_mass", d)


def bench_tsmm(dev):
    # demo/gpu_tsmm/main.cpp: ndofs = 125, ncells = 100000, two products, GFLOPs = 4*ncells*nd^2/t
    for ncells, nd in ((100000, 125), (1000000, 125), (1000000, 64), (2000000, 27), (300000, 216), (200000, 343)):
        xe = torch.rand(ncells * nd, dtype=torch.float64, device=dev)
        xq = torch.zeros_like(xe)
        ue = torch.zeros_like(xe)
        phi = torch.rand(nd, nd, dtype=torch.float64, device=dev)
        for layout in (0, 1):
            def two():
                w.tsmm(ncells, xe, phi, xq, layout=layout)
                w.tsmm(ncells, xq, phi, ue, layout=layout)
            ms = timeit(two)
            print(json.dumps({"op": f"TSMM x2 ({ncells} x {nd}) . ({nd} x {nd}), layout {layout}", "ms": round(ms, 4),
                              "GFLOPs": round(4.0 * ncells * nd * nd / ms / 1e6, 1),
                              "frac_of_f64_mfma_78.6TF": round(4.0 * ncells * nd * nd / ms / 1e9 / 78.6, 3),
                              "GBs": round(4 * 8.0 * ncells * nd / ms / 1e6, 1)}), flush=True)


def main():
    dev = torch.device("cuda", 0)
    only = sys.argv[1:] or ["stiffness", "mass", "dense", "vector"]
    if "tsmm" in only:
        bench_tsmm(dev)
        only = [o for o in only if o != "tsmm"]
        if not only:
            return
    if "tet-ab" in only:
        bench_tet_against(dev, os.environ["WAVEHIP_LIB_B"])
        only = [o for o in only if o != "tet-ab"]
        if not only:
            return
    if "cellform" in only:
        bench_cellform(dev)
        only = [o for o in only if o != "cellform"]
        if not only:
            return
    if "medium" in only:
        bench_medium(dev)
        only = [o for o in only if o != "medium"]
        if not only:
            return
    if "tet" in only:
        bench_tet(dev)
        only = [o for o in only if o != "tet"]
        if not only:
            return
    degrees = [int(v) for v in os.environ.get("DEGREES", "2,4,6").split(",")]
    for p in degrees:
        n = {1: 216, 2: 108, 3: 72, 4: 54, 5: 43, 6: 36, 7: 31}[p]     # ~10.2 M dofs each
        mesh = w.create_box(n)
        V = w.create_functionspace(mesh, p, build_dofmap=True)
        N = V.ndofs
        x = torch.rand(N, dtype=torch.float64, device=dev)
        y = torch.zeros(N, dtype=torch.float64, device=dev)
        tag = {"degree": p, "cells": mesh.ncells, "ndofs": N}
        if "stiffness" in only:
            cases = [(True, None), (False, None), (False, {"kernel": "batch"})]
            if "KS" in os.environ and p <= 4:
                cases = [(True, None), (True, {"variant": 3})]
            if p >= 5:   # the owner form on request next to the default k-split kernel (OWNER_VARIANTS=1: every cross-section)
                own = [{"update": "owner", "variant": v} for v in (0, 1, 2)] if "OWNER_VARIANTS" in os.environ else [{"update": "owner"}]
                cases[1:1] = [(True, t) for t in own]
            elif "KS" not in os.environ:   # per-cell geometry on request, next to the per-point dofmap operator
                cases[2:2] = [(False, {"geometry": "per_cell"}), (False, {"geometry": "per_cell", "metric": "full"})]
            cases = [c + (0,) for c in cases]
            if p in (4, 6):   # order-fixed accumulation next to the default dofmap operator
                cases.append((False, None, WF_FLAG_ORDERED))
            for structured, tuning, flags in cases:
                op = w.StiffnessOperator(V, p, structured=structured, tuning=tuning, flags=flags)
                report(f"stiffness P{p} " + ("box" if structured else "any dofmap") + f" [{op.kernel}]", timeit(lambda: op(x, y)),
                       op.alg_bytes(), N, dict(tag, kernel=op.kernel, geometry=op.geometry, metric=op.metric, update=op.update, lz=op.info.plan_lz,
                            tuning=str(tuning)))
                del op
        if "mass" in only:
            op = w.SpectralMassOperator(V, p, structured=False)
            report(f"lumped mass P{p} generic (fused gather*detJ->scatter)", timeit(lambda: op(x, y)), op.alg_bytes(), N, tag)
            del op
            op = w.SpectralMassOperator(V, p, structured=True)
            report(f"lumped mass P{p} box (pre-assembled diagonal)", timeit(lambda: op(x, y)), op.alg_bytes(), N, tag)
            del op
        if "dense" in only:
            pts, wts, D = w.tabulate_gll(p)
            # collocated GLL rule (demo/gpu_operator_monolithic) and Gauss rule of degree 2p (demo/gpu_operator)
            for label, (qp, qw), nodes in (("gll-collocated", (pts, wts), pts),
                                           ("equispaced+gauss", gl_rule(p + 1), np.linspace(0, 1, p + 1))):
                phi1 = lagrange(nodes, qp)
                m = len(qp)
                _, detq = w.precompute_geometric_data(mesh, p, use_fabs=False, clamp=False, want_G=False)
                if m != p + 1 or label != "gll-collocated":
                    # affine box: detJ = vol * w_q
                    W3 = np.einsum("k,j,i->kji", qw, qw, qw).reshape(-1)
                    detq = np.tile(W3 / mesh.ncells, (mesh.ncells, 1))
                op = w.MassOperator(V, p, phi1, detq)
                alg = mesh.ncells * (8.0 * m ** 3 + 4.0 * (p + 1) ** 3) + 16.0 * N
                report(f"dense mass P{p} {label} (sum-factorised Phi^T D Phi)", timeit(lambda: op.apply(x, y), reps=10),
                       alg, N, dict(tag, kernel=op.kernel, alg_bytes=alg, flops_ref_model=op.flops()))
                del op
                if label != "gll-collocated":   # order-fixed accumulation next to the default form
                    op = w.MassOperator(V, p, phi1, detq, flags=WF_FLAG_ORDERED)
                    report(f"dense mass P{p} {label} ordered [{op.kernel}]", timeit(lambda: op.apply(x, y), reps=10),
                           op.alg_bytes(), N, dict(tag, kernel=op.kernel, flops_ref_model=op.flops()))
                    del op
            bench_dense_rect(V, mesh, p, x, y, tag)
        if "vector" in only and p == 4:
            z = torch.zeros_like(x)
            report("axpy r=a*x+y", timeit(lambda: la.axpy(z, 0.5, x, y)), 24.0 * N, N)
            report("pointwise_div", timeit(lambda: la.pointwise_div(x, y, z)), 24.0 * N, N)
            report("copy", timeit(lambda: la.copy(x, z)), 16.0 * N, N)
            report("fill", timeit(lambda: la.fill(z, 0.0)), 8.0 * N, N)
        if "rk4" in only and p == 4:
            from wave_fenics_amd.linear_gll import LinearGLLOpt, cfl_time_step
            V.structured = True
            hi = (0.1, 0.1, 0.1)
            mesh2 = w.create_box(n, hi=hi)
            V2 = w.create_functionspace(mesh2, p, build_dofmap=False)
            dt, _ = cfl_time_step(mesh2, p, 1500.0, 0.5e6, CFL=0.25)
            for fused in (False, True):
                eqn = LinearGLLOpt(V2, p, 1500.0, 0.5e6, 6e4)
                eqn.init()
                run = eqn.rk4_fused if fused else eqn.rk4
                nwarm = 100 if float(os.environ.get("SETTLE", "1")) > 0 else 3   # past the power ramp after idle
                run(0.0, nwarm * dt - 1e-13, dt)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                nsteps = 50
                e0.record()
                run(nwarm * dt, (nwarm + nsteps) * dt - 1e-13, dt)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / nsteps
                print(json.dumps({"op": "RK4 time step P4 (4 stages: K + boundary + vector algebra) " + ("fused" if fused else "reference-order"),
                                  "ms_per_step": round(ms, 4), "Gdof_stages_per_s": round(4 * N / ms / 1e6, 2),
                                  "finite": bool(torch.isfinite(eqn.u_n).all())}), flush=True)
                del eqn
        del V, mesh, x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
