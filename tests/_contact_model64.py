"""A plain float64 statement of ONE contact evaluation (numpy, vectorised over contacts, no GPU).

Written from the formulas as this repository states them (dem-engine_amd/csrc/deme_force.h: calc_forces_body, hertz_full,
hertz_frictionless, side_contribution; oracle/deme_oracle.cpp: spheres_overlap, sphere_entity, calc_forces), with every
operation in float64 -- numpy's sqrt and / are correctly rounded.  Inputs are the fp32 / codec values the kernels read, widened.
tests/test_contact_zoo.py compares the oracle (fp32 reference arithmetic) and the HIP kernels with it contact by contact.
The sphere-triangle kind (KIND_TRI, tests/test_triangle_zoo.py) is written from the closest point on a triangle as Ericson states
it (Real-Time Collision Detection 5.1.5), not from csrc/deme_mesh.h: face region -> face normal and depth r - h, edge or vertex
region -> the direction from the closest point to the centre and depth r - distance; the contact point is the closest point.

Errors are measured relative to the per-contact SCALE  s = |k_n d| + |g_n v_n| + |k_t| |d_t| + |g_t| |v_t|  (the sum of the sizes
of the spring and damping terms), not to |F|: F is a sum of terms that cancel, by design in the separating class.
"""
import numpy as np

TINY = 1e-12          # DEME_TINY_FLOAT: the |tangential force| and |v_rot| guards (1e-24 on the squares in the fast kernels)
HUGE_RADIUS = float(np.float32(1e15))  # the radius an analytical object enters the model with
TWO_SQRT56 = 1.825741858350554
KIND_SPHERE, KIND_PLANE, KIND_CYL, KIND_TRI = 0, 1, 2, 3


def rot_matrix(q_wxyz):
    """(n, 3, 3): the nine coefficients of rot_coeffs (deme_device.h) -- the formula the kernels use, also for |q| != 1"""
    w, x, y, z = (np.asarray(q_wxyz, np.float64)[:, k] for k in range(4))
    R = np.empty((len(w), 3, 3))
    R[:, 0, 0] = 2.0 * (w * w + x * x) - 1.0
    R[:, 0, 1] = 2.0 * (x * y - w * z)
    R[:, 0, 2] = 2.0 * (x * z + w * y)
    R[:, 1, 0] = 2.0 * (x * y + w * z)
    R[:, 1, 1] = 2.0 * (w * w + y * y) - 1.0
    R[:, 1, 2] = 2.0 * (y * z - w * x)
    R[:, 2, 0] = 2.0 * (x * z - w * y)
    R[:, 2, 1] = 2.0 * (y * z + w * x)
    R[:, 2, 2] = 2.0 * (w * w + z * z) - 1.0
    return R


def _mv(R, v):
    return np.einsum("nij,nj->ni", R, v)


def _mtv(R, v):  # the conjugate quaternion's coefficients are the transposed ones
    return np.einsum("nji,nj->ni", R, v)


def _dot(a, b):
    return (a * b).sum(1)


def _len(a):
    return np.sqrt(_dot(a, a))


def pair_table(E, nu, CoR):
    """E_cnt, G_cnt, beta per material pair (nMat x nMat each) as the library's host code puts them in the table
    (deme_hip.hip: matProxy2ContactParam in fp32, beta = ln(CoR) / sqrt(ln(CoR)^2 + pi^2)), here in float64 from the fp32 inputs"""
    E, nu = np.asarray(E, np.float64), np.asarray(nu, np.float64)
    n = len(E)
    CoR = np.asarray(CoR, np.float64).reshape(n, n)
    a = (1.0 - nu * nu) / E
    g = 2.0 * (2.0 - nu) * (1.0 + nu) / E
    E_cnt = 1.0 / (a[:, None] + a[None, :])
    G_cnt = 1.0 / (g[:, None] + g[None, :])
    loge = np.where(CoR < TINY, np.log(TINY), np.log(np.maximum(CoR, 1e-300)))
    beta = loge / np.sqrt(loge * loge + np.pi ** 2)
    return E_cnt, G_cnt, beta


def coefficients(E_cnt, G_cnt, beta, mA, mB, rA, rB, depth):
    """k_n, gamma_n, k_t, gamma_t, mass_eff of the Hertzian model at overlap `depth` (> 0)"""
    m_eff = mA * mB / (mA + mB)
    sqrt_Rd = np.sqrt(depth * (rA * rB) / (rA + rB))
    Sn = 2.0 * E_cnt * sqrt_Rd
    k_n = (2.0 / 3.0) * Sn
    g_n = TWO_SQRT56 * beta * np.sqrt(Sn * m_eff)
    k_t = 8.0 * G_cnt * sqrt_Rd
    g_t = -TWO_SQRT56 * beta * np.sqrt(m_eff * k_t)
    return k_n, g_n, k_t, g_t, m_eff


def rolling_clock(E_cnt, beta, m_eff, rA, rB):
    """d_coeff and t_collision of the rolling-resistance branch (t_collision is nan where d_coeff >= 1)"""
    R_eff = np.sqrt((rA * rB) / (rA + rB))
    kn_s = (4.0 / 3.0) * E_cnt * np.sqrt(R_eff)
    gn_s = -2.0 * np.sqrt((5.0 / 3.0) * m_eff * E_cnt) * beta * R_eff ** 0.25
    d = gn_s / (2.0 * np.sqrt(kn_s * m_eff))
    with np.errstate(invalid="ignore", divide="ignore"):
        tc = np.where(d < 1.0, np.pi * np.sqrt(m_eff / (kn_s * (1.0 - d * d))), np.nan)
    return d, tc


def closest_point_on_triangle(A, B, C, P):
    """Ericson, Real-Time Collision Detection 5.1.5 (as tests/test_independent_pins.py states it), vectorised: the point of the
    triangle closest to P and its Voronoi region: 0 face, 1 / 2 / 3 vertex A / B / C, 4 / 5 / 6 edge AB / AC / BC"""
    ab, ac, bc = B - A, C - A, C - B
    ap, bp, cp = P - A, P - B, P - C
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    region = np.select(conds, [1, 2, 4, 3, 5, 6], 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = 1.0 / (va + vb + vc)
        pts = [A, B, A + (d1 / (d1 - d3))[:, None] * ab, C, A + (d2 / (d2 - d6))[:, None] * ac,
               B + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * bc, A + (vb * den)[:, None] * ab + (vc * den)[:, None] * ac]
    q = np.select([c[:, None] for c in conds], pts[:6], pts[6])
    return q, region


def geometry(c):
    """narrow phase in float64: touching, depth, normal (B2A), contact point, the owners' rotation matrices; for a triangle
    also the Voronoi region of the closest point and the signed height h of the sphere's centre over the face"""
    n = len(c["rA"])
    RA, RB = rot_matrix(c["qA"]), rot_matrix(c["qB"])
    bodyA = c["posA"] + _mv(RA, c["relA"])
    bodyB = c["posB"] + _mv(RB, c["relB"])
    kind = c["kind"]
    nrm, cp, depth = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    ss = kind == KIND_SPHERE
    if ss.any():  # spheres_overlap
        d = (bodyA - bodyB)[ss]
        dist = _len(d)
        u = d / dist[:, None]
        dep = c["rA"][ss] + c["rB"][ss] - dist
        nrm[ss], depth[ss] = u, dep
        cp[ss] = bodyB[ss] + (c["rB"][ss] - dep / 2.0)[:, None] * u
    dirw = _mv(RB, c["dirB"])
    pl = kind == KIND_PLANE
    if pl.any():  # sphere_entity, plane
        dist = _dot((bodyA - bodyB)[pl], dirw[pl])
        dep = c["rA"][pl] - dist
        nrm[pl], depth[pl] = dirw[pl], dep
        cp[pl] = bodyA[pl] - dirw[pl] * (dist + dep / 2.0)[:, None]
    cy = kind == KIND_CYL
    if cy.any():  # sphere_entity, infinite cylinder; sign +1: normal towards the axis
        s2c = (bodyB - bodyA)[cy]
        s2c = s2c - _dot(s2c, dirw[cy])[:, None] * dirw[cy]
        dr = _len(s2c)
        sg = c["signB"][cy]
        dep = c["rA"][cy] - sg * (c["sizeB"][cy] - dr)
        u = (sg / dr)[:, None] * s2c
        nrm[cy], depth[cy] = u, dep
        cp[cy] = bodyA[cy] - u * (c["rA"][cy] - dep / 2.0)[:, None]
    touching = ~(depth < -c["extra"])
    region, height = np.full(n, -1), np.full(n, np.nan)
    tr = kind == KIND_TRI
    if tr.any():  # sphere against one triangle: c["tri"] (n, 3, 3) holds the three nodes in the mesh owner's frame
        N = c["posB"][tr][:, None, :] + np.einsum("nij,nkj->nki", RB[tr], c["tri"][tr])
        A, B, C, P, r = N[:, 0], N[:, 1], N[:, 2], bodyA[tr], c["rA"][tr]
        q, reg = closest_point_on_triangle(A, B, C, P)
        fn = np.cross(B - A, C - A)
        fn /= _len(fn)[:, None]
        h = _dot(P - A, fn)
        d = P - q
        dist = _len(d)
        face = reg == 0
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.where(face[:, None], fn, d / dist[:, None])
        dep = np.where(face, r - h, r - dist)
        nrm[tr], depth[tr], cp[tr], region[tr], height[tr] = u, dep, q, reg, h
        # the extra margin counts on the positive side only; a sphere through the plane of the face with its centre a radius or
        # more away from that plane is no contact (the two-sided test of the reference's narrow phase)
        touching[tr] = ~((-dep > c["extra"][tr]) | ((dep > 0) & (np.abs(h) >= r)))
    return dict(touching=touching, depth=depth, normal=nrm, cp=cp, RA=RA, RB=RB, region=region, height=height)


def contact64(c, h, model="hertz"):
    """One contact evaluation per row of `c` (a dict of float64 arrays):
      posA, posB (n,3) decoded owner positions; qA, qB (n,4) w x y z; vA, vB; wA, wB body-frame angular velocities; mA, mB;
      relA, rA: A's component; kind (0 sphere, 1 plane, 2 cylinder, 3 triangle), relB, rB (sphere: component; else the object's
      position in its owner's frame and HUGE_RADIUS; triangle: zero and HUGE_RADIUS), dirB, sizeB, signB (object direction, cylinder
      radius, +1 inward / -1 outward); tri (n,3,3), only where a triangle occurs: its nodes in the frame of the mesh owner, which
      is the B side (posB, qB, vB, wB, mB);
      E_cnt, G_cnt, beta, mu, Crr: the material-pair entry; hist (n,4): delta_tan x/y/z, delta_time; extra: family extra margin.
    Returns a dict: touching, depth, normal, F (force on A), T (torque-only force), PA, PB (contact point in A's / B's body
    frame), hist (new), label, s (scale), kt, and the distances to the discontinuous thresholds (ft, vrot, clock, tc, d_coeff)."""
    g = geometry(c)
    n = len(c["rA"])
    RA, RB, nrm, depth, touching = g["RA"], g["RB"], g["normal"], g["depth"], g["touching"]
    PA = _mtv(RA, g["cp"] - c["posA"])
    PB = _mtv(RB, g["cp"] - c["posB"])
    F, T, hist = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 4))
    s, kt_out = np.zeros(n), np.zeros(n)
    ft_out, vrot_out, ftmax_out = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    clock_out, tc_out, dco_out = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    label = np.empty(n, dtype=object)
    label[~touching] = "apart"
    label[touching & ~(depth > 0)] = "margin"
    PA[~touching], PB[~touching] = 0.0, 0.0
    on = touching & (depth > 0)
    i = np.nonzero(on)[0]
    if len(i):
        d, u = depth[i], nrm[i]
        rvA = _mv(RA[i], np.cross(c["wA"][i], PA[i]))
        rvB = _mv(RB[i], np.cross(c["wB"][i], PB[i]))
        vel = (c["vA"][i] + rvA) - (c["vB"][i] + rvB)
        proj = _dot(vel, u)
        k_n, g_n, k_t, g_t, m_eff = coefficients(c["E_cnt"][i], c["G_cnt"][i], c["beta"][i], c["mA"][i], c["mB"][i], c["rA"][i],
                                                 c["rB"][i], d)
        Fn = k_n * d + g_n * proj
        f = Fn[:, None] * u
        sc = np.abs(k_n * d) + np.abs(g_n * proj)
        lab = np.where(Fn < 0, "separating", "normal_only").astype(object)
        kt_out[i] = k_t
        if model == "hertz":
            vt = vel - proj[:, None] * u
            dt = c["hist"][i, :3] + h * vt
            dt = dt - _dot(dt, u)[:, None] * u
            clock = c["hist"][i, 3] + h
            mu, Crr = c["mu"][i], c["Crr"][i]
            # rolling resistance
            dco, tc = rolling_clock(c["E_cnt"][i], c["beta"][i], m_eff, c["rA"][i], c["rB"][i])
            has_r = Crr > 0
            young = has_r & (dco < 1.0) & (clock <= np.where(np.isnan(tc), np.inf, tc))
            roll = has_r & ~young
            vrot = rvB - rvA
            vmag = _len(vrot)
            turn = roll & (vmag > TINY)
            tq = np.zeros_like(f)
            with np.errstate(invalid="ignore", divide="ignore"):
                tq[turn] = (vrot[turn] / vmag[turn, None]) * (Crr[turn] * _len(f[turn]))[:, None]
            # friction
            has_t = mu > 0
            tf = -k_t[:, None] * dt - g_t[:, None] * vt
            ft = _len(tf)
            ft_max = np.abs(Fn) * mu
            live = has_t & (ft > TINY)
            slip = live & (ft > ft_max)
            with np.errstate(invalid="ignore", divide="ignore"):
                tf_c = (ft_max / ft)[:, None] * tf
            dt_c = (tf_c + g_t[:, None] * vt) / (-k_t[:, None])
            tf = np.where(slip[:, None], tf_c, tf)
            dt = np.where(slip[:, None], dt_c, dt)
            tf[~live] = 0.0
            f = f + tf
            sc = sc + np.where(has_t, np.abs(k_t) * _len(dt) + np.abs(g_t) * _len(vt), 0.0)
            lab[live & ~slip & (Fn >= 0)] = "stick"
            lab[slip & (Fn >= 0)] = "slip"
            lab[young] = "roll_young"
            lab[roll & (dco < 1.0)] = "roll_on"
            lab[roll & ~(dco < 1.0)] = "roll_on_dcoeff"
            lab[roll & ~turn] = "roll_norot"
            T[i] = tq
            hist[i, :3], hist[i, 3] = dt, clock
            ft_out[i] = np.where(has_t, ft, np.nan)
            ftmax_out[i] = np.where(has_t, ft_max, np.nan)
            vrot_out[i] = np.where(roll, vmag, np.nan)
            clock_out[i], tc_out[i], dco_out[i] = np.where(has_r, clock, np.nan), np.where(has_r, tc, np.nan), np.where(has_r, dco, np.nan)
        F[i], s[i], label[i] = f, sc, lab
    return dict(touching=touching, depth=depth, normal=nrm, F=F, T=T, PA=PA, PB=PB, hist=hist, label=label, s=s, kt=kt_out,
                ft=ft_out, vrot=vrot_out, clock=clock_out, tc=tc_out, d_coeff=dco_out, RA=RA, RB=RB,
                region=g["region"], height=g["height"], ft_max=ftmax_out)


def owner_sums64(out, ownerA, ownerB, n_owners, mass, moi, mB_side, gravity=(0.0, 0.0, 0.0)):
    """Per-owner linear and body-frame angular acceleration from the per-contact outputs, in float64: a = sum(+-F / m) + g,
    alpha = sum(locCP x R^T (+-(F + T))) / MOI (side_contribution in deme_force.h; the integrator adds gravity: k_integrate).
    mass, moi: per owner; mB_side: the mass the B side divides by (an analytical object's own).  Also returns the per-contact
    contributions of the two sides ((aA, alA), (aB, alB)) and the per-owner sums of s / m and of |r| s / MOI (the scales)."""
    F, tot = out["F"], out["F"] + out["T"]
    aA = F / mass[ownerA][:, None]
    aB = -F / mB_side[:, None]
    alA = np.cross(out["PA"], _mtv(out["RA"], tot)) / moi[ownerA]
    alB = np.cross(out["PB"], _mtv(out["RB"], -tot)) / moi[ownerB]
    a, al = np.zeros((n_owners, 3)), np.zeros((n_owners, 3))
    sa, sl = np.zeros(n_owners), np.zeros(n_owners)
    for own, ca, cl, m, P in ((ownerA, aA, alA, mass[ownerA], out["PA"]), (ownerB, aB, alB, mB_side, out["PB"])):
        np.add.at(a, own, ca)
        np.add.at(al, own, cl)
        np.add.at(sa, own, out["s"] / m)
        np.add.at(sl, own, out["s"] * _len(P) / moi[own].min(1))
    a = a + np.asarray(gravity, np.float64)[None, :]
    return a, al, (aA, alA), (aB, alB), sa, sl
