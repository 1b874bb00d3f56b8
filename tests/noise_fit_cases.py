"""NumPy restatements of the two kernels of the noise fit (include/ste.h: ste_ukf_noise_moments_f64, ste_ukf_noise_mstep_f64;
DESIGN.md, "Noise fit") with the orders of evaluation the header fixes, so that the device's results are compared bit for bit,
and an EM for R on the pinned oracle (oracle.ukf_oracle.forward_track / backward_track, test_ukf_loglik.restate_track for the
log-likelihood) that the device's fit is held against."""
import numpy as np

from oracle import ukf_oracle as orc

TRACK_NAN, TRACK_NOT_FINITE = 0x1, 0x2
GROUP_EMPTY, GROUP_BAD_VARIANCE, GROUP_BAD_MEMBER = 0x1, 0x2, 0x4
STRUCTURES = {"scalar": 0, "diag2": 1, "block2": 2}
STATUS_NAN = 0x1


def tri(r, c):
    """index of (r, c) in a packed upper triangle: 00 01 02 03 11 12 13 22 23 33"""
    r, c = min(r, c), max(r, c)
    return r * 4 - (r * (r - 1)) // 2 + (c - r)


def wrap180(a):
    return (a + 180.0) % 360.0 - 180.0


def restate_moments(H, nsteps, upd_idx, z, sm_mean, sm_cov, status=None):
    """ste_ukf_noise_moments_f64 on arrays in the device's layout (track index last): upd_idx (Nmax, B), z (Tmax, 4, B),
    sm_mean (Nmax+1, 4, B), sm_cov (Nmax+1, 10 or 16, B).  Returns moments (10, B), count (B,), vsum (4, B), track_status (B,).
    Every product and sum is one float64 operation, in the header's order."""
    H = np.asarray(H, dtype=np.float64)
    Nmax, B = upd_idx.shape
    Tmax = z.shape[0]
    packed = sm_cov.shape[1] == 10
    mom, cnt, vsum, tst = np.zeros((10, B)), np.zeros(B, dtype=np.int32), np.zeros((4, B)), np.zeros(B, dtype=np.int32)
    f = np.float64
    with np.errstate(all="ignore"):
        for t in range(B):
            if status is not None and status[t] & STATUS_NAN:
                tst[t] = TRACK_NAN
                continue
            ns = min(max(int(nsteps[t]), 0), Nmax)
            S, vs, n, finite = [f(0.0)] * 10, [f(0.0)] * 4, 0, True
            for k in range(ns):
                ui = int(upd_idx[k, t])
                if not 0 <= ui < Tmax:
                    continue
                m = [f(sm_mean[k + 1, c, t]) for c in range(4)]
                P = lambda i, c: f(sm_cov[k + 1, tri(i, c) if packed else min(i, c) * 4 + max(i, c), t])  # noqa: E731
                v = []
                for r in range(4):
                    hm = ((H[r, 0] * m[0] + H[r, 1] * m[1]) + H[r, 2] * m[2]) + H[r, 3] * m[3]
                    v.append(f(z[ui, r, t]) - hm)
                v[3] = wrap180(v[3])
                for r in range(4):
                    G = [((H[r, 0] * P(0, c) + H[r, 1] * P(1, c)) + H[r, 2] * P(2, c)) + H[r, 3] * P(3, c) for c in range(4)]
                    for c in range(r, 4):
                        gh = ((G[0] * H[c, 0] + G[1] * H[c, 1]) + G[2] * H[c, 2]) + G[3] * H[c, 3]
                        term = v[r] * v[c] + gh
                        finite = finite and bool(np.isfinite(term))
                        S[tri(r, c)] = S[tri(r, c)] + term
                vs = [vs[c] + v[c] for c in range(4)]
                n += 1
            if not finite:
                tst[t] = TRACK_NOT_FINITE
                continue
            mom[:, t], cnt[t], vsum[:, t] = S, n, vs
    return mom, cnt, vsum, tst


def wave_sum(values):
    """The sum of a group's members as ste_ukf_noise_mstep_f64 forms it: lane l adds members l, l + 64, ... from 0.0, then
    for off = 32 .. 1 lane l < off adds lane l + off's value."""
    lanes = [np.float64(0.0)] * 64
    with np.errstate(all="ignore"):
        for i, x in enumerate(values):
            lanes[i % 64] = lanes[i % 64] + np.float64(x)
        off = 32
        while off >= 1:
            for lane in range(off):
                lanes[lane] = lanes[lane] + lanes[lane + off]
            off //= 2
    return lanes[0]


def project(s00, s01, s11, n, structure):
    """(r00, r01, r11) and the group's status from the sums and the count."""
    with np.errstate(all="ignore"):
        dn = np.float64(n)
        m00, m01, m11 = np.float64(s00) / dn, np.float64(s01) / dn, np.float64(s11) / dn
        if structure == "scalar":
            r00 = r11 = (m00 + m11) / np.float64(2.0)
            r01 = np.float64(0.0)
        elif structure == "diag2":
            r00, r01, r11 = m00, np.float64(0.0), m11
        else:
            r00, r01, r11 = m00, m01, m11
    st = GROUP_EMPTY if n == 0 else 0
    if not (r00 > 0.0 and np.isfinite(r00) and r11 > 0.0 and np.isfinite(r11) and np.isfinite(r01)):
        st |= GROUP_BAD_VARIANCE
    return (r00, r01, r11), st


def restate_mstep(moments, count, offsets, members, structure, R_tracks):
    """ste_ukf_noise_mstep_f64: ``offsets`` / ``members`` None = every track a group of its own.  Returns R_group (10, G),
    n_group (G,), group_status (G,) and the new R_tracks (10, B)."""
    B = moments.shape[1]
    if offsets is None:
        groups, lane_per_track = [[t] for t in range(B)], True
    else:
        groups, lane_per_track = [list(members[offsets[g]:offsets[g + 1]]) for g in range(len(offsets) - 1)], False
    G = len(groups)
    Rg, ng, gs, Rt = np.zeros((10, G)), np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32), np.array(R_tracks, dtype=np.float64)
    for g, mem in enumerate(groups):
        if lane_per_track:
            s = [np.float64(0.0) + moments[e, mem[0]] for e in (0, 1, 4)]
        else:
            s = [wave_sum(moments[e, mem]) for e in (0, 1, 4)]
        n = int(np.sum(count[mem], dtype=np.int64))
        (r00, r01, r11), st = project(s[0], s[1], s[2], n, structure)
        Rg[[0, 1, 4], g], ng[g], gs[g] = (r00, r01, r11), n, st
        if not st & (GROUP_EMPTY | GROUP_BAD_VARIANCE):
            Rt[:, mem] = Rg[:, g:g + 1]
    return Rg, ng, gs, Rt


# ----------------------------------------------------------------------------------------------------------------
# EM on the oracle
# ----------------------------------------------------------------------------------------------------------------
def oracle_e_step(sb, b, substeps, H, Q, R, P0):
    """Track b of a synthetic batch under R: (loglik, sum |l_u|, moments (4, 4) summed over its updates, number of updates).
    The update after step k produced history row k + 1; the initial update is not one of them (row 0 is the prior)."""
    from test_ukf_loglik import restate_track

    dt = np.repeat(sb.dts[b] / substeps, substeps)
    z = sb.z[b]
    lik = restate_track(z[:, 0], P0, H, Q, R, dt, sb.dts[b], z, sb.sog_rate[b], sb.cog_rate[b])
    means, covs = orc.forward_track(z[:, 0], P0, H, Q, R, dt, sb.dts[b], z, sb.sog_rate[b], sb.cog_rate[b])
    sm, sP = orc.backward_track(means, covs, Q, dt, len(sb.dts[b]), sb.sog_rate[b], sb.cog_rate[b])
    fires, zidx = orc.update_schedule(dt, sb.dts[b])
    M, n = np.zeros((4, 4)), 0
    for k in np.flatnonzero(fires):
        v = z[:, zidx[k]] - H @ sm[k + 1]
        v[3] = wrap180(v[3])
        M += np.outer(v, v) + H @ sP[k + 1] @ H.T
        n += 1
    return lik["loglik"], lik["abs"], M, n


def project_matrix(M, structure):
    R = np.zeros((4, 4))
    if structure == "scalar":
        R[0, 0] = R[1, 1] = 0.5 * (M[0, 0] + M[1, 1])
    elif structure == "diag2":
        R[0, 0], R[1, 1] = M[0, 0], M[1, 1]
    else:
        R[:2, :2] = M[:2, :2]
    return R


def oracle_em(sb, substeps, H, Q, R0, P0, groups, structure, iterations):
    """``iterations`` M-steps from R0 for every group of ``groups`` (a list of lists of track indices), Q fixed.  Returns
    R (iterations + 1, G, 4, 4) -- iterate 0 is R0 --, loglik (iterations + 1, G) of every iterate (one more E-step scores the
    last) and the sums of |l_u| (iterations + 1, G) that the likelihood's tolerance is relative to."""
    G = len(groups)
    R = [np.stack([np.asarray(R0, dtype=np.float64)] * G)]
    ll, ab = np.zeros((iterations + 1, G)), np.zeros((iterations + 1, G))
    for it in range(iterations + 1):
        new = np.zeros((G, 4, 4))
        for g, mem in enumerate(groups):
            M, n = np.zeros((4, 4)), 0
            for b in mem:
                l, a, Mb, nb = oracle_e_step(sb, b, substeps, H, Q, R[it][g], P0)
                ll[it, g] += l
                ab[it, g] += a
                M += Mb
                n += nb
            new[g] = project_matrix(M / n, structure)
        if it < iterations:
            R.append(new)
    return np.stack(R), ll, ab
