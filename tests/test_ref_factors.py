"""CPU, three legs: the REFERENCE'S OWN cost functors (lidarFactor.hpp, ceres_cost_function.h compiled unmodified into oracle/_ref/libref.so,
stand-in Eigen / Ceres Jet in oracle/ref_shim/) vs the oracle's restatement (oracle/orc_factors.h through orc.eval_lidar_factor /
orc.eval_vo_factor) vs the product header include/vloam_hip/factors.hpp (tests/cpp/factors_probe.cpp) — residuals and Jacobians.

The reference returns Jacobians in the ambient 4 + 3 parameters; the oracle returns them in the tangent space Ceres solves in, so the
reference's are projected with EigenQuaternionParameterization's plus-Jacobian, written out below from its formula
(Plus(x, delta) = q_delta * x with q_delta = [delta, 1] to first order — delta on the LEFT, as Ceres' EigenQuaternionParameterization
computes it; its ComputeJacobian is d/d delta = [[w, z, -y], [-z, w, x], [y, -x, w], [-x, -y, -z]] for x = (x, y, z, w)).  The product header is
compared in the ambient parameters, where a wrong slerp branch shows most (d/dw of the slerp weights is 0 in the linear branch, O(1) in
the spherical one).

HOW INDEPENDENT THE LEGS ARE.  The reference functors, their long-double yardstick AND the factors.hpp probe are all differentiated by
the same dual number, oracle/ref_shim/ceres/jet.h: a wrong derivative rule there (in acos, in operator/) would be common to both sides of
test_product_header_functor_against_the_reference_functor and to E.  That leg therefore pins factors.hpp's EXPRESSIONS to the reference's,
not the derivative rules.  The oracle leg is the independent one for derivatives: it differentiates with oracle/orc_ceres.h's Jet, which
shares no code with the stand-in, and the oracle's Jacobians are in turn checked against central differences in tests/test_oracle_math.py.

TOLERANCE.  Not chosen by hand: the reference functor evaluated in double is compared with the same functor in long double
(Jet<long double, N>) over the same inputs; that is the double evaluation's own rounding error E.  The oracle and factors.hpp compute the
same expressions in another order, so they must lie within 8 E of the reference's double result, and never looser than the 1e-9 that the
GPU tests grant the kernel against the oracle.  All differences are scaled: max |a - b| / max(1, max |b|) over one evaluation's residuals,
and the same over its Jacobian.  Measured on this file's inputs (g++ 11.4, x86-64, -O3 -ffp-contract=off):

    functor                E residual   E Jacobian    bound = min(8 E, 1e-9): residual / Jacobian
    LidarEdgeFactor        1.5e-10      9.1e-09       1e-09 / 1e-09
    LidarPlaneFactor       6.5e-15      8.1e-09       5.2e-14 / 1e-09
    LidarPlaneNormFactor   8.9e-15      7e-16         7.1e-14 / 5.6e-15
    LidarDistanceFactor    6.6e-15      2e-16         5.3e-14 / 1.6e-15
    CostFunctor33          1.1e-14      1.1e-10       8.8e-14 / 8.8e-10
    CostFunctor32          5.6e-15      5.4e-11       4.5e-14 / 4.3e-10
    CostFunctor23          6.2e-15      7.9e-11       5e-14 / 6.3e-10
    CostFunctor22          9.3e-16      8.6e-11       7.4e-15 / 6.9e-10

(The edge and plane factors' E is dominated by the deliberately near-degenerate inputs: edges with |lpa - lpb| down to 1e-7 m divide by that
length, and quaternions a few ulps beside the slerp threshold take acos / sin of an angle of 1e-8.  Their 8 E exceeds 1e-9, so 1e-9 holds.)

CostFunctor33 / CostFunctor23 / LidarDistanceFactor: the oracle and factors.hpp do not provide them.  The reference's solve path never
creates the first two (visual_odometry.cpp:333-340 and :383-390 are commented out; only CostFunctor32, :361, and CostFunctor22, :408, are
added to the problem); LidarDistanceFactor is created only inside blocks of laser_mapping.cpp that are commented out (:531, :595).  They are
still evaluated here so that the harness covers all eight: double against long double (same Jet on both sides), residuals against a plain
numpy long-double formula under the derived residual bound, and for LidarDistanceFactor the Jacobian against its closed form under the
derived Jacobian bound.  The Jacobians of CostFunctor33 / CostFunctor23 have no check independent of the stand-in Jet; the same
AngleAxisRotatePoint text is differentiated independently through CostFunctor32 / CostFunctor22 in the oracle leg.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ref   # oracle/ref.py, a module of this repository (conftest puts oracle/ on the path): if it does not import, that is an error, not a skip

pytestmark = pytest.mark.skipif(not ref.available(), reason=ref.SKIP_REASON)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def quat_near_identity(rng, dist):
    """(x, y, z, w) at rotation-vector distance ~dist from the identity (dist = 0: exactly the identity)."""
    if dist == 0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    ax = unit(rng.standard_normal(3)) * np.sin(dist / 2)
    return np.array([ax[0], ax[1], ax[2], np.cos(dist / 2)])


def quat_with_w(rng, w):
    """Unit-ish quaternion whose w is EXACTLY the given double (the slerp threshold looks at w alone when the other side is the identity)."""
    v = unit(rng.standard_normal(3)) * np.sqrt(max(1.0 - w * w, 0.0))
    return np.array([v[0], v[1], v[2], w])


def lidar_inputs(seed, n=300):
    """(payload pieces, q, t, s) for the LiDAR functors: realistic geometry + the edges of slerp and of the edge factor's denominator."""
    rng = np.random.default_rng(seed)
    out = []
    one = 1.0 - EPS
    special_q = [quat_near_identity(rng, 0), quat_near_identity(rng, 1e-9), quat_near_identity(rng, 1e-4), quat_near_identity(rng, 1e-4),
                 quat_with_w(rng, np.nextafter(1.0, 0.0)), quat_with_w(rng, one), quat_with_w(rng, np.nextafter(one, 0.0)),      # linear | linear | spherical
                 quat_with_w(rng, 1.0 - 1e-12), quat_near_identity(rng, 3e-8), -quat_near_identity(rng, 0.3)]                   # ..., d < 0: scale1 negated
    special_s = [0.0, 1e-12, 0.5, 1.0, 1.0 + 1e-9, 1.02]
    for i in range(n + len(special_q) * len(special_s)):
        cp = rng.uniform(-40, 40, 3) * np.array([1, 1, 0.1])
        a = cp + rng.uniform(-1.0, 1.0, 3)
        sep = rng.uniform(0.05, 2.0) if i % 10 else rng.uniform(1e-7, 1e-4)      # near-degenerate edges: |lpa - lpb| small
        b = a + unit(rng.standard_normal(3)) * sep
        j = cp + rng.uniform(-1.0, 1.0, 3)
        l = j + rng.uniform(-2.0, 2.0, 3)
        m = j + rng.uniform(-2.0, 2.0, 3)
        nrm = unit(rng.standard_normal(3))
        d = -float(nrm @ (cp + rng.uniform(-0.3, 0.3, 3)))
        if i < n:
            q = quat_near_identity(rng, rng.uniform(0.0, 0.2) if i % 7 else rng.uniform(0.0, 3.0))
            s = 1.0 if i % 3 else rng.uniform(0.0, 1.0)
        else:
            k = i - n
            q, s = special_q[k // len(special_s)], special_s[k % len(special_s)]
        t = rng.uniform(-2, 2, 3)
        out.append(dict(cp=cp, a=a, b=b, j=j, l=l, m=m, nrm=nrm, d=d, q=q, t=t, s=s, closed=cp + rng.uniform(-1, 1, 3)))
    return out


def vo_inputs(seed, n=300):
    rng = np.random.default_rng(seed)
    out = []
    tiny = np.sqrt(EPS)    # AngleAxisRotatePoint switches at theta^2 > eps, i.e. |angles| > sqrt(eps) = 1.49e-8
    special = [np.zeros(3), unit(rng.standard_normal(3)) * tiny * 0.99, unit(rng.standard_normal(3)) * tiny * 1.01, unit(rng.standard_normal(3)) * 1e-12,
               unit(rng.standard_normal(3)) * 1e-6, unit(rng.standard_normal(3)) * 3.0]
    for i in range(n + len(special)):
        X0 = np.array([rng.uniform(-20, 20), rng.uniform(-3, 3), rng.uniform(4, 60)])
        ang = unit(rng.standard_normal(3)) * rng.uniform(0, 0.1) if i < n else special[i - n]
        t = rng.uniform(-1.5, 1.5, 3)
        X1 = X0 + rng.uniform(-0.5, 0.5, 3)
        out.append(dict(X0=X0, X1=X1, x0b=X0[:2] / X0[2], x1b=X1[:2] / X1[2], ang=ang, t=t))
    return out


def payload(name, c):
    if name == "LidarEdgeFactor":
        return np.concatenate([c["cp"], c["a"], c["b"], [c["s"]]])
    if name == "LidarPlaneFactor":
        return np.concatenate([c["cp"], c["j"], c["l"], c["m"], [c["s"]]])
    if name == "LidarPlaneNormFactor":
        return np.concatenate([c["cp"], c["nrm"], [c["d"]]])
    if name == "LidarDistanceFactor":
        return np.concatenate([c["cp"], c["closed"]])
    if name == "CostFunctor33":
        return np.concatenate([c["X0"], c["X1"]])
    if name == "CostFunctor32":
        return np.concatenate([c["X0"], c["x1b"]])
    if name == "CostFunctor23":
        return np.concatenate([c["x0b"], c["X1"]])
    if name == "CostFunctor22":
        return np.concatenate([c["x0b"], c["x1b"]])
    raise KeyError(name)


TYPE = {v[0]: k for k, v in ref.FACTORS.items()}
LIDAR = ["LidarEdgeFactor", "LidarPlaneFactor", "LidarPlaneNormFactor", "LidarDistanceFactor"]
VO = ["CostFunctor33", "CostFunctor32", "CostFunctor23", "CostFunctor22"]


def cases(name):
    if name in LIDAR:
        return [(payload(name, c), c["q"], c["t"], c) for c in lidar_inputs(100 + TYPE[name])]
    return [(payload(name, c), c["ang"], c["t"], c) for c in vo_inputs(200 + TYPE[name])]


def scaled(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def plus_jacobian(q):
    x, y, z, w = q
    return np.array([[w, z, -y], [-z, w, x], [y, -x, w], [-x, -y, -z]])


def to_tangent(J, q):
    """[nres, 4 + 3] ambient -> [nres, 3 + 3]: what Ceres assembles with EigenQuaternionParameterization on block 0."""
    return np.concatenate([J[:, :4] @ plus_jacobian(q), J[:, 4:]], axis=1)


def measure(name):
    """max over this file's inputs of the scaled difference between the reference functor in double and in long double."""
    er = ej = 0.0
    for pay, p0, p1, _ in cases(name):
        r, J = ref.eval_factor(TYPE[name], pay, p0, p1)
        rl, Jl = ref.eval_factor(TYPE[name], pay, p0, p1, long_double=True)
        assert np.isfinite(r).all() and np.isfinite(J).all(), (name, pay, p0, p1)
        er, ej = max(er, scaled(r, rl)), max(ej, scaled(J, Jl))
    return er, ej


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """include/vloam_hip/factors.hpp behind the harness's C entry (tests/cpp/factors_probe.cpp), with the oracle's compiler flags."""
    so = tmp_path_factory.mktemp("factors_probe") / "libfactors_probe.so"
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-shared",
                           "-I", os.path.join(ROOT, "oracle", "ref_shim"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "factors_probe.cpp"), "-o", str(so)])
    L = C.CDLL(str(so))
    L.fac_eval_factor.argtypes = [C.c_int] + [C.c_void_p] * 5

    def ev(name, pay, p0, p1):
        _, nres, n0, _ = ref.FACTORS[TYPE[name]]
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (pay, p0, p1)]
        r, J = np.zeros(3), np.zeros(3 * (n0 + 3))
        n = L.fac_eval_factor(TYPE[name], *[v.ctypes.data_as(C.c_void_p) for v in a], r.ctypes.data_as(C.c_void_p), J.ctypes.data_as(C.c_void_p))
        assert n == nres, (name, n)
        return r[:n], J[:n * (n0 + 3)].reshape(n, n0 + 3)
    return ev


@pytest.mark.parametrize("name", LIDAR + VO)
def test_measured_double_error_is_what_the_header_says(name):
    """The table in this file's header stays honest: the measured E of every functor is within the value the bounds were derived from."""
    er, ej = measure(name)
    print("%-22s E residual %.3g, E Jacobian %.3g" % (name, er, ej))
    assert er <= MEASURED[name][0] and ej <= MEASURED[name][1]


@pytest.mark.parametrize("name", ["LidarEdgeFactor", "LidarPlaneFactor", "LidarPlaneNormFactor", "CostFunctor32", "CostFunctor22"])
def test_oracle_functor_against_the_reference_functor(orc, name):
    br, bj = bound(name)
    worst = [0.0, 0.0]
    for pay, p0, p1, c in cases(name):
        r, J = ref.eval_factor(TYPE[name], pay, p0, p1)
        if name in LIDAR:
            geom = {"LidarEdgeFactor": np.concatenate([c["a"], c["b"]]), "LidarPlaneFactor": np.concatenate([c["j"], c["l"], c["m"]]),
                    "LidarPlaneNormFactor": np.concatenate([c["nrm"], [c["d"]]])}[name]
            ro, Jo = orc.eval_lidar_factor(TYPE[name], c["cp"], geom, p0, p1, s=c.get("s", 1.0))
            J = to_tangent(J, p0)
        else:
            ro, Jo = orc.eval_vo_factor({"CostFunctor32": 3, "CostFunctor22": 4}[name], pay, p0, p1)
        dr, dj = scaled(ro, r), scaled(Jo, J)
        worst = [max(worst[0], dr), max(worst[1], dj)]
        assert dr <= br and dj <= bj, "%s: oracle vs reference %.3g (bound %.3g) / Jacobian %.3g (bound %.3g) at q/angles %r s %r" % (name, dr, br, dj, bj, p0, c.get("s"))
    print("%-22s oracle vs reference: residual %.3g (bound %.3g), tangent Jacobian %.3g (bound %.3g)" % (name, worst[0], br, worst[1], bj))


@pytest.mark.parametrize("name", ["LidarEdgeFactor", "LidarPlaneFactor", "LidarPlaneNormFactor", "CostFunctor32", "CostFunctor22"])
def test_product_header_functor_against_the_reference_functor(probe, name):
    br, bj = bound(name)
    worst = [0.0, 0.0]
    for pay, p0, p1, c in cases(name):
        r, J = ref.eval_factor(TYPE[name], pay, p0, p1)
        rp, Jp = probe(name, pay, p0, p1)
        dr, dj = scaled(rp, r), scaled(Jp, J)
        worst = [max(worst[0], dr), max(worst[1], dj)]
        assert dr <= br and dj <= bj, "%s: factors.hpp vs reference %.3g (bound %.3g) / Jacobian %.3g (bound %.3g) at q/angles %r s %r" % (name, dr, br, dj, bj, p0, c.get("s"))
    print("%-22s factors.hpp vs reference: residual %.3g (bound %.3g), ambient Jacobian %.3g (bound %.3g)" % (name, worst[0], br, worst[1], bj))


def test_product_header_has_no_functor_the_solve_path_does_not_use(probe):
    """CostFunctor33 / CostFunctor23 / LidarDistanceFactor: not in factors.hpp (see this file's header for the reference lines)."""
    src = open(os.path.join(ROOT, "include", "vloam_hip", "factors.hpp")).read()
    for name in ("CostFunctor33", "CostFunctor23", "LidarDistanceFactor"):
        assert "struct " + name not in src


def _rodrigues(a):
    a = np.asarray(a, dtype=np.longdouble)
    th = np.sqrt(a @ a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=np.longdouble)
    if th == 0:
        return np.eye(3, dtype=np.longdouble) + K
    return np.eye(3, dtype=np.longdouble) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * (K @ K)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=np.longdouble)


@pytest.mark.parametrize("name", ["LidarDistanceFactor", "CostFunctor33", "CostFunctor23"])
def test_functors_without_a_counterpart_against_a_plain_formula(name):
    """Residuals of the three functors nothing else restates, against numpy long double, under the bounds derived in the header:
    q * p + t - c with Eigen's q * p = p + 2 w (u x p) + 2 u x (u x p) (any q, unit or not), R(a) X0 + t - X1, and the projection residual of
    R(a)^T (X1 - t).  LidarDistanceFactor's Jacobian against the closed form of that expression:
    d/du = -2 w [p]x + 2 ((u . p) I + u p^T - 2 p u^T), d/dw = 2 u x p, d/dt = I."""
    br, bj = bound(name)
    L = np.longdouble
    for pay, p0, p1, c in cases(name):
        r, J = ref.eval_factor(TYPE[name], pay, p0, p1)
        if name == "LidarDistanceFactor":
            u, w, p = np.asarray(p0[:3], dtype=L), L(p0[3]), c["cp"].astype(L)
            uxp = _cross(u, p)
            want = p + 2 * w * uxp + 2 * _cross(u, uxp) + p1.astype(L) - c["closed"].astype(L)
            px = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]], dtype=L)
            Ju = -2 * w * px + 2 * ((u @ p) * np.eye(3, dtype=L) + np.outer(u, p) - 2 * np.outer(p, u))
            Jw = np.concatenate([Ju, (2 * uxp)[:, None], np.eye(3, dtype=L)], axis=1)
            assert scaled(J, Jw) <= bj, (name, p0, scaled(J, Jw), bj)
        elif name == "CostFunctor33":
            want = _rodrigues(p0) @ c["X0"].astype(L) + p1.astype(L) - c["X1"].astype(L)
        else:
            v = _rodrigues(p0).T @ (c["X1"].astype(L) - p1.astype(L))
            want = np.array([v[0] - v[2] * L(c["x0b"][0]), v[1] - v[2] * L(c["x0b"][1])])
        assert scaled(r, want) <= br, (name, p0, scaled(r, want), br)


# ---- measured E (see the header table) and the bounds derived from it
MEASURED = {
    "LidarEdgeFactor": (1.5e-10, 9.1e-09),
    "LidarPlaneFactor": (6.5e-15, 8.1e-09),
    "LidarPlaneNormFactor": (8.9e-15, 7e-16),
    "LidarDistanceFactor": (6.6e-15, 2e-16),
    "CostFunctor33": (1.1e-14, 1.1e-10),
    "CostFunctor32": (5.6e-15, 5.4e-11),
    "CostFunctor23": (6.2e-15, 7.9e-11),
    "CostFunctor22": (9.3e-16, 8.6e-11),
}


def bound(name):
    er, ej = MEASURED[name]
    return min(8 * er, 1e-9), min(8 * ej, 1e-9)
