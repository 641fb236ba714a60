"""The clipped PPO loss of include/macm.h (macm_policy_logp, macm_ppo_loss, macm_ppo_grad) in numpy float64,
written from the definition and not from the kernels (tests/ only).

Every function works on float32 inputs converted to float64, one numpy operation per operation of the
definition, in its association. numpy's exp and log and the device library's differ by a few 2^-53 relative,
so the comparison with the device needs bounds, and the bounds need magnitudes; `loss` returns them beside
the values:

    S_dlogits[r, q] = k (|adv| ratio + c_e (1 + max_c |lp_hc|))      k = scale / rows
    S_dvalues[r]    = k c_v (|v| + |ret| + |old_v|)
    S_logp[r]       = max_q |z[r, q]|
    stat_mag[i]     = the mean over rows of the summed magnitudes of the operands of the stat's last line

An element of logp, dlogits or dvalues passes within one float32 ulp of the float32 rounding of the reference
or within 2^-44 S (about 256 float64 roundings of a value of size S); a stat within (rows + 64) 2^-52 stat_mag
(at most `rows` roundings in the sums, and slack for the row terms' own error).

A row is "undecided" where a branch of the definition hangs on a comparison that those few 2^-53 could turn:
|ratio - (1 +- clip)| < 2^-40, or |u - c| < 2^-40 (u + c) with u != c. The seeded inputs below have none
(tests/test_ppo_ref.py asserts it), so the GPU tests compare every row."""
import numpy as np

F32, F64 = np.float32, np.float64
STATS = ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_frac", "ratio_max", "rows")
EDGE = 2.0 ** -40


def heads(logits, actions):
    """p, lp [rows, 3, 3], Hh [rows, 3], logp [rows] (float64) of float32 logits [rows, 9], uint8 actions [rows, 3]"""
    z = np.asarray(logits, F32).astype(F64).reshape(-1, 3, 3)
    a = np.asarray(actions).reshape(-1, 3).astype(np.int64)
    m = z.max(axis=2, keepdims=True)
    e = np.exp(z - m)
    S = ((e[..., 0] + e[..., 1]) + e[..., 2])[..., None]
    lse = m + np.log(S)
    lp = z - lse
    p = e / S
    pl = p * lp
    Hh = -((pl[..., 0] + pl[..., 1]) + pl[..., 2])
    taken = np.take_along_axis(lp, a[..., None], axis=2)[..., 0]
    logp = (taken[:, 0] + taken[:, 1]) + taken[:, 2]
    return p, lp, Hh, logp


def log_prob(logits, actions):
    """(logp, entropy, S_logp): float64 values before their rounding to float32, and logp's magnitude"""
    _, _, Hh, logp = heads(logits, actions)
    S = np.abs(np.asarray(logits, F32).astype(F64)).reshape(-1, 9).max(axis=1)
    return logp, (Hh[:, 0] + Hh[:, 1]) + Hh[:, 2], S


def loss(logits=None, actions=None, old_logp=None, adv=None, values=None, ret=None, old_values=None, clip=0.2,
         vf_coef=0.5, ent_coef=0.01, vf_clip=None, scale=1.0):
    """A dict: dlogits [rows, 9], dvalues [rows], stats [8] (float64, unrounded), their magnitudes S_dlogits,
    S_dvalues, stat_mag [8], the row quantities ratio, g_logp, and `undecided` [rows] (bool)."""
    rows = len(logits) if logits is not None else len(values)
    eps, cv, ce = F64(F32(clip)), F64(F32(vf_coef)), F64(F32(ent_coef))
    k = F64(F32(scale)) / F64(rows)
    out = dict(rows=rows, undecided=np.zeros(rows, bool))
    st, mag = np.zeros(8), np.zeros(8)
    if logits is not None:
        p, lp, Hh, logp = heads(logits, actions)
        A = np.asarray(adv, F32).astype(F64)
        ratio = np.exp(logp.astype(F32).astype(F64) - np.asarray(old_logp, F32).astype(F64))
        lo, hi = 1.0 - eps, 1.0 + eps
        s1, s2 = ratio * A, np.minimum(np.maximum(ratio, lo), hi) * A
        unclipped = s1 <= s2
        pl = -np.where(unclipped, s1, s2)
        g = np.where(unclipped, -A * ratio, 0.0)
        H = (Hh[:, 0] + Hh[:, 1]) + Hh[:, 2]
        logr = np.log(ratio)
        kl = (ratio - 1.0) - logr
        clipped = np.abs(ratio - 1.0) > eps
        ind = (np.arange(3)[None, None, :] == np.asarray(actions).reshape(-1, 3, 1)).astype(F64)
        d = k * (g[:, None, None] * (ind - p) + ce * (p * (lp + Hh[:, :, None])))
        out.update(dlogits=d.reshape(rows, 9), ratio=ratio, g_logp=g, logp=logp,
                   S_dlogits=np.repeat(k * (np.abs(A)[:, None] * ratio[:, None]
                                            + ce * (1.0 + np.abs(lp).max(axis=2))), 3, axis=1))
        out["undecided"] |= (np.abs(ratio - lo) < EDGE) | (np.abs(ratio - hi) < EDGE)
        st[1], st[3], st[4], st[5], st[6] = pl.mean(), H.mean(), kl.mean(), clipped.mean(), ratio.max()
        mag[1] = (np.abs(s1) + np.abs(s2)).mean()
        mag[3] = np.abs(p * lp).sum(axis=(1, 2)).mean()
        mag[4] = (1.0 + ratio + np.abs(logr)).mean()
        mag[6] = ratio.max()  # (not a sum: stats_close takes 64 x 2^-52 of it)
    if values is not None:
        v, R = np.asarray(values, F32).astype(F64), np.asarray(ret, F32).astype(F64)
        dv = v - R
        u = dv * dv
        vl, gv = 0.5 * u, dv
        S = np.abs(v) + np.abs(R)
        mag[2] = u.mean()
        if old_values is not None:
            ov, ev = np.asarray(old_values, F32).astype(F64), F64(F32(vf_clip))
            diff = v - ov
            dc = (ov + np.minimum(np.maximum(diff, -ev), ev)) - R
            c = dc * dc
            vl = 0.5 * np.maximum(u, c)
            gv = np.where(u >= c, dv, np.where(np.abs(diff) <= ev, dc, 0.0))
            S = S + np.abs(ov)
            mag[2] = (u + c).mean()
            out["undecided"] |= (u != c) & (np.abs(u - c) < EDGE * (u + c))
        out.update(dvalues=k * (cv * gv), S_dvalues=k * cv * S)
        st[2] = vl.mean()
    st[0] = (st[1] + cv * st[2]) - ce * st[3]
    mag[0] = mag[1] + cv * mag[2] + ce * mag[3]
    st[7] = rows
    out.update(stats=st, stat_mag=mag)
    return out


def close(got, want, S):
    """Per element: got (float32) within one float32 ulp of float32(want), or within 2^-44 S of want"""
    got = np.asarray(got, F32)
    w32 = np.asarray(want, F64).astype(F32)
    ulp = np.spacing(np.abs(w32))
    return (np.abs(got.astype(F64) - w32.astype(F64)) <= ulp.astype(F64)) | \
        (np.abs(got.astype(F64) - want) <= 2.0 ** -44 * S)


def stats_close(got, ref):
    """Per stat: within (rows + 64) 2^-52 of its magnitude (ratio_max, one row's exp and no sum: 64 x 2^-52 of
    itself); clip_frac and rows exact"""
    tol = (ref["rows"] + 64) * 2.0 ** -52 * ref["stat_mag"]
    tol[6] = 64 * 2.0 ** -52 * ref["stat_mag"][6]
    ok = np.abs(np.asarray(got, F64) - ref["stats"]) <= tol
    ok[5] = got[5] == ref["stats"][5]
    ok[7] = got[7] == ref["stats"][7]
    return ok


# ---- the seeded inputs the tests share ---------------------------------------------------------------
ROWS = (1, 63, 64, 65, 129, 4097, 131137)
PAST_CAP = 256 * 2048 + 257  # more rows than macm_ppo_loss's largest grid has threads: the second trip of its loop
VF_CLIP = 0.2


def inputs(rows, seed=0):
    """A dict of float32 / uint8 arrays: logits 2 N(0, 1) with saturated rows (+-80) and heads of three equal
    logits among them, old_logp around the logits' own logp (ratios on both sides of the clip range), adv,
    values, ret N(0, 1), old_values around values (differences on both sides of VF_CLIP)."""
    rng = np.random.default_rng([seed + 7000, rows])
    logits = (2.0 * rng.standard_normal((rows, 9))).astype(F32)
    sat = np.arange(rows) % 11 == 3
    logits[sat] = rng.choice(np.array([-80.0, 80.0], F32), (int(sat.sum()), 9))
    logits[np.arange(rows) % 13 == 5, 3:6] = F32(0.75)
    actions = rng.integers(0, 3, (rows, 3)).astype(np.uint8)
    logp = heads(logits, actions)[3]
    old_logp = (logp + 0.3 * rng.standard_normal(rows)).astype(F32)
    values = rng.standard_normal(rows).astype(F32)
    return dict(logits=logits, actions=actions, old_logp=old_logp, adv=rng.standard_normal(rows).astype(F32),
                values=values, ret=rng.standard_normal(rows).astype(F32),
                old_values=(values + 0.3 * rng.standard_normal(rows)).astype(F32))
