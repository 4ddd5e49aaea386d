"""CPU reference for the compressing SNARK on BN254 G1 (include/lurk_hip.h, "the compressing SNARK on BN254 G1"): the sum-checks of
oracle/spartan_ref.py / oracle/spartan_fast.py over Fr, step for step up to the squeeze of gamma, then a HyperKZG opening of the joint
polynomial (tests/hyperkzg_ref.py) with its challenges bound to the same Keccak transcript.  Python integers only.

The prover knows the trapdoor tau of its key ck[i] = [tau^i]G (a commitment is one scalar multiple), and a proof is valid iff the
verifier accepts so far AND ``hyperkzg_ref.trapdoor_holds(tau, L, R)``: no pairing is needed.  ``verify`` / ``verify_batched`` are the
header's verifiers check for check, with the LURK_VERIFY_* codes."""
from __future__ import annotations

import random

from oracle import pyref as R
from oracle import spartan_ref as S
from oracle.keccak_transcript import KeccakTranscript
from tests import bn254_ref as BN
from tests import hyperkzg_ref as HK

Q = BN.BN254_R
CURVE = BN.BN254
ACCEPTED, MALFORMED, OUTER, INNER, BATCH, OPENING = 0, 1, 2, 3, 4, 5  # LURK_VERIFY_*
LABEL = b"lurk-hip spartan v2bn254"  # what the provers of lurk_beta_amd/spartan_kzg.py pass as the transcript's label
LABEL_BATCHED = LABEL + b"/batched"


def commit(tau: int, v) -> tuple | None:
    return HK.commit_trapdoor(tau, [x % Q for x in v])


# ---- instances ------------------------------------------------------------------------------------------------------------------------
def product_instance(num_cons: int, num_vars: int, nio: int, seed: int, folded: bool):
    """tests/test_oracle_spartan.product_instance over Fr, for any pair of sizes: row i < nprod is (random combination of free variables,
    u, X) * (another) = its own product variable; the rows past the product variables (num_cons > num_vars - nfree) have an empty B and C,
    0 = 0.  Returns mats, X, u, W, E - strict (u = 1, E = 0) or, folded, the relaxed fold of two strict instances (u != 1, E != 0)."""
    q = Q
    rng = random.Random(seed)
    nfree = max(1, num_vars - num_cons)
    nprod = min(num_cons, num_vars - nfree)
    assert nprod >= 1 and 1 + nio <= num_vars
    cols = list(range(nfree)) + [num_vars + k for k in range(1 + nio)]  # free variables, u, X

    def rand_mat(rows):
        indptr, indices, data = [0], [], []
        for i in range(num_cons):
            if i < rows:
                for c in rng.sample(cols, rng.randint(1, min(3, len(cols)))):
                    indices.append(c)
                    data.append(rng.choice([1, q - 1, 2, rng.randrange(q)]))
            indptr.append(len(indices))
        return indptr, indices, data

    A, B = rand_mat(num_cons), rand_mat(nprod)
    Cm = ([min(i, nprod) for i in range(num_cons + 1)], [nfree + i for i in range(nprod)], [1] * nprod)
    mats = (A, B, Cm)

    def fresh(s):
        r2 = random.Random(s)
        free = [r2.randrange(q) for _ in range(nfree)]
        X = [r2.randrange(q) for _ in range(nio)]
        z = free + [0] * (num_vars - nfree) + [1] + X + [0] * (num_vars - 1 - nio)
        az, bz, _ = S.matrices_times(q, mats, z)
        return free + [a * b % q for a, b in zip(az[:nprod], bz[:nprod])] + [0] * (num_vars - nfree - nprod), X

    W2, X2 = fresh(seed + 1)
    if not folded:
        return mats, X2, 1, W2, [0] * num_cons
    W1, X1 = fresh(seed + 2)
    z1 = W1 + [1] + X1 + [0] * (num_vars - 1 - nio)
    z2 = W2 + [1] + X2 + [0] * (num_vars - 1 - nio)
    m1, m2 = S.matrices_times(q, mats, z1), S.matrices_times(q, mats, z2)
    T = R.cross_term(q, *m1, *m2, 1, 1)
    r = rng.randrange(1, q)
    W = [(a + r * b) % q for a, b in zip(W1, W2)]
    X = [(a + r * b) % q for a, b in zip(X1, X2)]
    return mats, X, (1 + r) % q, W, [r * t % q for t in T]


def is_sat(mats, X, u, W, E) -> bool:
    nv = len(W)
    z = list(W) + [u] + list(X) + [0] * (nv - 1 - len(X))
    az, bz, cz = S.matrices_times(Q, mats, z)
    return all((a * b - u * c - e) % Q == 0 for a, b, c, e in zip(az, bz, cz, E))


# ---- the opening over the transcript ----------------------------------------------------------------------------------------------------
def _kzg_challenge(tr: KeccakTranscript):
    def challenge(stage, data):
        if stage == 1:
            tr.absorb_scalars(b"kzg_v", data)
            return tr.squeeze(b"kzg_q", Q)
        for pt in data:
            tr.absorb_point(b"kzg_com" if stage == 0 else b"kzg_W", pt)
        return tr.squeeze(b"kzg_r" if stage == 0 else b"kzg_d", Q)

    return challenge


def _open(tr, tau, polys, gamma, evals, r_z, N):
    """joint = sum_k gamma^k pad_N(P_k) opened at r_z; the opening's value must be the batched claim"""
    joint = [0] * N
    for k, p in enumerate(polys):
        g = pow(gamma, k, Q)
        for j, a in enumerate(p):
            joint[j] = (joint[j] + g * a) % Q
    pf = HK.prove(tau, joint, r_z, _kzg_challenge(tr))
    assert pf["y"] == sum(pow(gamma, k, Q) * e for k, e in enumerate(evals)) % Q, "the opening's value differs from the batched claim"
    return dict(kzg_com=pf["com"], kzg_v=[e for row in pf["v"] for e in row], kzg_w=pf["w"])


def _check_opening(tr, ell, comm_joint, y, r_z, proof):
    """-> (L, R, accepted, failed_check): the three challenges in the prover's order, then HyperKZG's verifier up to the pairing"""
    ch = _kzg_challenge(tr)
    r = ch(0, proof["kzg_com"])
    if r == 0:
        return None, None, False, MALFORMED
    q = ch(1, proof["kzg_v"])
    d = ch(2, proof["kzg_w"])
    v = [proof["kzg_v"][t * ell:(t + 1) * ell] for t in range(3)]
    L, Rr, ok, code = HK.pairing_inputs(ell, comm_joint, r_z, y, proof["kzg_com"], v, proof["kzg_w"], r, q, d)
    if ok:
        return L, Rr, True, ACCEPTED
    return None, None, False, MALFORMED if code == HK.MALFORMED else OPENING


def _wellformed(scalars, points) -> bool:
    in_fq = lambda p: p is None or (len(p) == 2 and all(isinstance(c, int) and 0 <= c < BN.BN254_P for c in p))
    return all(isinstance(s, int) and 0 <= s < Q for s in scalars) and all(in_fq(p) and CURVE.on_curve(p) for p in points)


def _flat(rows):
    return [c for row in rows for c in row]


def _eq_at(x, y):
    acc = 1
    for a, b in zip(x, y):
        acc = acc * ((a * b + (1 - a) * (1 - b)) % Q) % Q
    return acc


def _rounds(tr, degree, claim, tables, rounds):
    """a sum-check over the transcript, one round at a time (the challenge depends on the round polynomial)"""
    polys, rs = [], []
    for _ in range(rounds):
        poly = R.sumcheck_prove(Q, claim, tables, [0])[0][0]
        tr.absorb_scalars(b"p", poly)
        r = tr.squeeze(b"c", Q)
        polys.append(poly)
        rs.append(r)
        claim = R.unipoly_eval(Q, poly, r)
        tables = [R.bind_top(Q, t, r) for t in tables]
    return polys, rs, tables


def _replay(tr, polys):
    rs = []
    for poly in polys:
        tr.absorb_scalars(b"p", poly)
        rs.append(tr.squeeze(b"c", Q))
    return rs


def _sparse_at(mats, eq_rx, eq_ry, r):
    abc = 0
    for k, (indptr, indices, data) in enumerate(mats):
        acc = 0
        for i in range(len(indptr) - 1):
            for j in range(indptr[i], indptr[i + 1]):
                acc += data[j] * eq_rx[i] * eq_ry[indices[j]]
        abc = (abc + pow(r, k, Q) * acc) % Q
    return abc


# ---- single instance ------------------------------------------------------------------------------------------------------------------
def prove(tau: int, mats, num_cons: int, num_vars: int, X, comm_W, comm_E, u: int, W, E, label: bytes = LABEL) -> dict:
    """oracle/spartan_ref.py: prove up to gamma (same labels and order), then the HyperKZG opening.  Points are (x, y) tuples / None."""
    q = Q
    ell_x, ell_y = num_cons.bit_length() - 1, num_vars.bit_length()
    N = max(num_cons, num_vars)
    ell = N.bit_length() - 1
    assert ell >= 1
    tr = KeccakTranscript(label)
    tr.absorb_point(b"comm_W", comm_W)
    tr.absorb_point(b"comm_E", comm_E)
    tr.absorb_scalars(b"uX", [u] + list(X))
    z = S._pad(list(W) + [u] + list(X), 2 * num_vars)
    Az, Bz, Cz = S.matrices_times(q, mats, z)
    tau_pt = [tr.squeeze(b"t", q) for _ in range(ell_x)]
    uCzE = [(u * c + e) % q for c, e in zip(Cz, E)]
    polys_outer, r_x, tables = _rounds(tr, 3, 0, [R.eq_evals(q, tau_pt), Az, Bz, uCzE], ell_x)
    claim_Az, claim_Bz = tables[1][0], tables[2][0]
    claim_Cz, eval_E = S.mle_eval(q, Cz, r_x), S.mle_eval(q, E, r_x)
    tr.absorb_scalars(b"claims_outer", [claim_Az, claim_Bz, claim_Cz, eval_E])
    r = tr.squeeze(b"r", q)
    claim_inner = (claim_Az + r * claim_Bz + r * r * claim_Cz) % q
    eA, eB, eC = S.matrices_transposed_times(q, mats, R.eq_evals(q, r_x), 2 * num_vars)
    abc = [(a + r * b + r * r * c) % q for a, b, c in zip(eA, eB, eC)]
    polys_inner, r_y, _ = _rounds(tr, 2, claim_inner, [abc, z], ell_y)
    eval_W = S.mle_eval(q, W, r_y[1:])
    tr.absorb_scalars(b"eval_W", [eval_W])
    P1, P2 = S._pad(W, N), S._pad(E, N)
    x1 = [0] * (ell - (ell_y - 1)) + r_y[1:]
    x2 = [0] * (ell - ell_x) + r_x
    rho = tr.squeeze(b"rho", q)

    def sq_batch(poly):
        tr.absorb_scalars(b"p", poly)
        return tr.squeeze(b"c", q)

    polys_batch, r_z, finals, _ = S.sumcheck_prove_quad_batch(q, [eval_W, eval_E], [(R.eq_evals(q, x1), P1), (R.eq_evals(q, x2), P2)], [1, rho], sq_batch)
    evals_batch = [finals[0][1], finals[1][1]]
    tr.absorb_scalars(b"evals_batch", evals_batch)
    gamma = tr.squeeze(b"gamma", q)
    proof = dict(polys_outer=polys_outer, claims_outer=[claim_Az, claim_Bz, claim_Cz], eval_E=eval_E, polys_inner=polys_inner, eval_W=eval_W,
                 polys_batch=polys_batch, evals_batch=evals_batch)
    proof.update(_open(tr, tau, [W, E], gamma, evals_batch, r_z, N))
    return proof


def verify(mats, num_cons: int, num_vars: int, X, comm_W, comm_E, u: int, proof: dict, label: bytes = LABEL):
    """-> (L, R, accepted, failed_check); L = R = None unless accepted so far."""
    q = Q
    ell_x, ell_y = num_cons.bit_length() - 1, num_vars.bit_length()
    N = max(num_cons, num_vars)
    ell = N.bit_length() - 1
    rej = lambda code: (None, None, False, code)
    try:
        shapes_ok = ([len(p) for p in proof["polys_outer"]] == [4] * ell_x and [len(p) for p in proof["polys_inner"]] == [3] * ell_y and
                     [len(p) for p in proof["polys_batch"]] == [3] * ell and len(proof["claims_outer"]) == 3 and len(proof["evals_batch"]) == 2 and
                     len(proof["kzg_com"]) == ell - 1 and len(proof["kzg_v"]) == 3 * ell and len(proof["kzg_w"]) == 3)
        scalars = ([u] + list(X) + _flat(proof["polys_outer"]) + list(proof["claims_outer"]) + [proof["eval_E"]] + _flat(proof["polys_inner"]) + [proof["eval_W"]] +
                   _flat(proof["polys_batch"]) + list(proof["evals_batch"]) + list(proof["kzg_v"]))
        points = [comm_W, comm_E] + list(proof["kzg_com"]) + list(proof["kzg_w"])
    except (KeyError, TypeError):
        return rej(MALFORMED)
    if not shapes_ok or not _wellformed(scalars, points):
        return rej(MALFORMED)
    tr = KeccakTranscript(label)
    tr.absorb_point(b"comm_W", comm_W)
    tr.absorb_point(b"comm_E", comm_E)
    tr.absorb_scalars(b"uX", [u] + list(X))
    tau_pt = [tr.squeeze(b"t", q) for _ in range(ell_x)]
    r_x = _replay(tr, proof["polys_outer"])
    final = S._sc_verify(q, 0, proof["polys_outer"], r_x)
    claim_Az, claim_Bz, claim_Cz = proof["claims_outer"]
    eval_E = proof["eval_E"]
    if final is None or final != _eq_at(tau_pt, r_x) * (claim_Az * claim_Bz - u * claim_Cz - eval_E) % q:
        return rej(OUTER)
    tr.absorb_scalars(b"claims_outer", [claim_Az, claim_Bz, claim_Cz, eval_E])
    r = tr.squeeze(b"r", q)
    claim_inner = (claim_Az + r * claim_Bz + r * r * claim_Cz) % q
    r_y = _replay(tr, proof["polys_inner"])
    final = S._sc_verify(q, claim_inner, proof["polys_inner"], r_y)
    eval_W = proof["eval_W"]
    abc = _sparse_at(mats, R.eq_evals(q, r_x), R.eq_evals(q, r_y), r)
    eval_X = S.mle_eval(q, S._pad([u] + list(X), num_vars), r_y[1:])
    eval_z = ((1 - r_y[0]) * eval_W + r_y[0] * eval_X) % q
    if final is None or final != abc * eval_z % q:
        return rej(INNER)
    tr.absorb_scalars(b"eval_W", [eval_W])
    x1 = [0] * (ell - (ell_y - 1)) + r_y[1:]
    x2 = [0] * (ell - ell_x) + r_x
    rho = tr.squeeze(b"rho", q)
    r_z = _replay(tr, proof["polys_batch"])
    final = S._sc_verify(q, (eval_W + rho * eval_E) % q, proof["polys_batch"], r_z)
    pw, pe = proof["evals_batch"]
    if final is None or final != (_eq_at(x1, r_z) * pw + rho * _eq_at(x2, r_z) * pe) % q:
        return rej(BATCH)
    tr.absorb_scalars(b"evals_batch", [pw, pe])
    gamma = tr.squeeze(b"gamma", q)
    comm_joint = CURVE.add(comm_W, CURVE.mul(gamma, comm_E))
    return _check_opening(tr, ell, comm_joint, (pw + gamma * pe) % q, r_z, proof)


# ---- batched --------------------------------------------------------------------------------------------------------------------------
def _pad_factor(r_pad) -> int:
    acc = 1
    for r in r_pad:
        acc = acc * ((1 - r) % Q) % Q
    return acc


def _batch_dims(insts):
    ell_x = max(it["num_cons"] for it in insts).bit_length() - 1
    ell_y = max(it["num_vars"] for it in insts).bit_length()
    N = max(max(it["num_cons"], it["num_vars"]) for it in insts)
    return ell_x, ell_y, N, N.bit_length() - 1


def _batch_round(tr, claim, groups, coeffs, cubic):
    """one round of a sum-check shared by several table groups through `coeffs`: (poly, challenge, bound groups)"""
    evs = [0] * (4 if cubic else 3)
    for c, tabs in zip(coeffs, groups):
        h = len(tabs[0]) // 2
        for pt in ([0, 2, 3] if cubic else [0, 2]):
            acc = 0
            for i in range(h):
                vals = [(t[i] + pt * (t[h + i] - t[i])) % Q for t in tabs]
                acc += vals[0] * (vals[1] * vals[2] - vals[3]) if cubic else vals[0] * vals[1]
            evs[pt] = (evs[pt] + c * acc) % Q
    evs[1] = (claim - evs[0]) % Q
    poly = R.unipoly_from_evals(Q, evs)
    tr.absorb_scalars(b"p", poly)
    r = tr.squeeze(b"c", Q)
    return poly, r, [[R.bind_top(Q, t, r) for t in tabs] for tabs in groups]


def _batch_prologue(tr, insts):
    tr.absorb_scalars(b"n", [len(insts)])
    for it in insts:
        tr.absorb_point(b"comm_W", it["comm_W"])
        tr.absorb_point(b"comm_E", it["comm_E"])
        tr.absorb_scalars(b"uX", [it["u"]] + list(it["X"]))


def prove_batched(tau: int, insts: list[dict], label: bytes = LABEL_BATCHED) -> dict:
    """oracle/spartan_fast.py: prove_batched up to gamma in Python integers, then the HyperKZG opening of sum_k gamma^k pad_N(P_k) over
    (W_0, E_0, W_1, ...).  insts[i]: dict(mats, num_cons, num_vars, X, u, W, E, comm_W, comm_E)."""
    q, n = Q, len(insts)
    ell_x, ell_y, N, ell = _batch_dims(insts)
    tr = KeccakTranscript(label)
    _batch_prologue(tr, insts)
    tau_pt = [tr.squeeze(b"t", q) for _ in range(ell_x)]
    rho_o = tr.squeeze(b"rho_outer", q)
    eq_tau = R.eq_evals(q, tau_pt)
    zs, czs, groups = [], [], []
    for it in insts:
        nv = it["num_vars"]
        z = S._pad(list(it["W"]) + [it["u"]] + list(it["X"]), 2 * nv)
        Az, Bz, Cz = S.matrices_times(q, it["mats"], z)
        uCzE = [(it["u"] * c + e) % q for c, e in zip(Cz, it["E"])]
        zs.append(z)
        czs.append(Cz)
        groups.append([eq_tau] + [S._pad(t, 1 << ell_x) for t in (Az, Bz, uCzE)])
    co = [pow(rho_o, i, q) for i in range(n)]
    polys_outer, r_x, claim = [], [], 0
    for _ in range(ell_x):
        poly, r, groups = _batch_round(tr, claim, groups, co, True)
        polys_outer.append(poly)
        r_x.append(r)
        claim = R.unipoly_eval(q, poly, r)
    eq_rx = R.eq_evals(q, r_x)
    claims_outer, evals_E = [], []
    for it, tabs, Cz in zip(insts, groups, czs):
        nc = it["num_cons"]
        px = ell_x - (nc.bit_length() - 1)
        claims_outer.append([tabs[1][0], tabs[2][0], sum(a * b for a, b in zip(Cz, eq_rx[:nc])) % q])
        evals_E.append(S.mle_eval(q, it["E"], r_x[px:]))
    tr.absorb_scalars(b"claims_outer", _flat(claims_outer) + evals_E)
    r = tr.squeeze(b"r", q)
    rho_i = tr.squeeze(b"rho_inner", q)
    groups, claims_inner = [], []
    for it, z, cl in zip(insts, zs, claims_outer):
        nc, nv = it["num_cons"], it["num_vars"]
        eA, eB, eC = S.matrices_transposed_times(q, it["mats"], eq_rx[:nc], 2 * nv)
        abc = [(a + r * b + r * r * c) % q for a, b, c in zip(eA, eB, eC)]
        groups.append([S._pad(abc, 1 << ell_y), S._pad(z, 1 << ell_y)])
        claims_inner.append((cl[0] + r * cl[1] + r * r * cl[2]) % q)
    ci = [pow(rho_i, i, q) for i in range(n)]
    claim = sum(c * e for c, e in zip(ci, claims_inner)) % q
    polys_inner, r_y = [], []
    for _ in range(ell_y):
        poly, rr, groups = _batch_round(tr, claim, groups, ci, False)
        polys_inner.append(poly)
        r_y.append(rr)
        claim = R.unipoly_eval(q, poly, rr)
    evals_W = [S.mle_eval(q, it["W"], r_y[ell_y - it["num_vars"].bit_length() + 1:]) for it in insts]
    tr.absorb_scalars(b"evals_W", evals_W)
    polys, points, claims = [], [], []
    for it, eW, eE in zip(insts, evals_W, evals_E):
        nc, nv = it["num_cons"], it["num_vars"]
        py, px = ell_y - nv.bit_length(), ell_x - (nc.bit_length() - 1)
        polys += [list(it["W"]), list(it["E"])]
        points += [[0] * (ell - (nv.bit_length() - 1)) + r_y[py + 1:], [0] * (ell - (nc.bit_length() - 1)) + r_x[px:]]
        claims += [eW, eE]
    rho = tr.squeeze(b"rho", q)
    cb = [pow(rho, k, q) for k in range(2 * n)]
    groups = [[R.eq_evals(q, x), S._pad(p, N)] for x, p in zip(points, polys)]
    claim = sum(c * e for c, e in zip(cb, claims)) % q
    polys_batch, r_z = [], []
    for _ in range(ell):
        poly, rr, groups = _batch_round(tr, claim, groups, cb, False)
        polys_batch.append(poly)
        r_z.append(rr)
        claim = R.unipoly_eval(q, poly, rr)
    evals_batch = [g[1][0] for g in groups]
    tr.absorb_scalars(b"evals_batch", evals_batch)
    gamma = tr.squeeze(b"gamma", q)
    proof = dict(polys_outer=polys_outer, claims_outer=claims_outer, evals_E=evals_E, polys_inner=polys_inner, evals_W=evals_W, polys_batch=polys_batch,
                 evals_batch=evals_batch)
    proof.update(_open(tr, tau, polys, gamma, evals_batch, r_z, N))
    return proof


def verify_batched(insts: list[dict], proof: dict, label: bytes = LABEL_BATCHED):
    """insts[i]: dict(mats, num_cons, num_vars, X, u, comm_W, comm_E).  -> (L, R, accepted, failed_check)"""
    q, n = Q, len(insts)
    ell_x, ell_y, N, ell = _batch_dims(insts)
    rej = lambda code: (None, None, False, code)
    try:
        shapes_ok = ([len(p) for p in proof["polys_outer"]] == [4] * ell_x and [len(p) for p in proof["polys_inner"]] == [3] * ell_y and
                     [len(p) for p in proof["polys_batch"]] == [3] * ell and [len(c) for c in proof["claims_outer"]] == [3] * n and
                     len(proof["evals_E"]) == n and len(proof["evals_W"]) == n and len(proof["evals_batch"]) == 2 * n and
                     len(proof["kzg_com"]) == ell - 1 and len(proof["kzg_v"]) == 3 * ell and len(proof["kzg_w"]) == 3)
        scalars = (_flat([[it["u"]] + list(it["X"]) for it in insts]) + _flat(proof["polys_outer"]) + _flat(proof["claims_outer"]) + list(proof["evals_E"]) +
                   _flat(proof["polys_inner"]) + list(proof["evals_W"]) + _flat(proof["polys_batch"]) + list(proof["evals_batch"]) + list(proof["kzg_v"]))
        points = _flat([[it["comm_W"], it["comm_E"]] for it in insts]) + list(proof["kzg_com"]) + list(proof["kzg_w"])
    except (KeyError, TypeError):
        return rej(MALFORMED)
    if not shapes_ok or not _wellformed(scalars, points):
        return rej(MALFORMED)
    tr = KeccakTranscript(label)
    _batch_prologue(tr, insts)
    tau_pt = [tr.squeeze(b"t", q) for _ in range(ell_x)]
    rho_o = tr.squeeze(b"rho_outer", q)
    r_x = _replay(tr, proof["polys_outer"])
    final = S._sc_verify(q, 0, proof["polys_outer"], r_x)
    tau_rx = _eq_at(tau_pt, r_x)
    want = 0
    for i, (it, (cA, cB, cC), eE) in enumerate(zip(insts, proof["claims_outer"], proof["evals_E"])):
        px = ell_x - (it["num_cons"].bit_length() - 1)
        want = (want + pow(rho_o, i, q) * tau_rx % q * (cA * cB - it["u"] * cC - _pad_factor(r_x[:px]) * eE)) % q
    if final is None or final != want:
        return rej(OUTER)
    tr.absorb_scalars(b"claims_outer", _flat(proof["claims_outer"]) + list(proof["evals_E"]))
    r = tr.squeeze(b"r", q)
    rho_i = tr.squeeze(b"rho_inner", q)
    claim_inner = sum(pow(rho_i, i, q) * (cA + r * cB + r * r * cC) for i, (cA, cB, cC) in enumerate(proof["claims_outer"])) % q
    r_y = _replay(tr, proof["polys_inner"])
    final = S._sc_verify(q, claim_inner, proof["polys_inner"], r_y)
    eq_rx, eq_ry = R.eq_evals(q, r_x), R.eq_evals(q, r_y)
    want = 0
    for i, (it, eW) in enumerate(zip(insts, proof["evals_W"])):
        nc, nv = it["num_cons"], it["num_vars"]
        py = ell_y - nv.bit_length()
        abc = _sparse_at(it["mats"], eq_rx[:nc], eq_ry[: 2 * nv], r)
        eval_X = S.mle_eval(q, S._pad([it["u"]] + list(it["X"]), nv), r_y[py + 1:])
        t = r_y[py]
        want = (want + pow(rho_i, i, q) * abc % q * (_pad_factor(r_y[:py]) * (((1 - t) * eW + t * eval_X) % q) % q)) % q
    if final is None or final != want:
        return rej(INNER)
    tr.absorb_scalars(b"evals_W", list(proof["evals_W"]))
    points, claims, comms = [], [], []
    for it, eW, eE in zip(insts, proof["evals_W"], proof["evals_E"]):
        nc, nv = it["num_cons"], it["num_vars"]
        py, px = ell_y - nv.bit_length(), ell_x - (nc.bit_length() - 1)
        points += [[0] * (ell - (nv.bit_length() - 1)) + r_y[py + 1:], [0] * (ell - (nc.bit_length() - 1)) + r_x[px:]]
        claims += [eW, eE]
        comms += [it["comm_W"], it["comm_E"]]
    rho = tr.squeeze(b"rho", q)
    r_z = _replay(tr, proof["polys_batch"])
    final = S._sc_verify(q, sum(pow(rho, k, q) * e for k, e in enumerate(claims)) % q, proof["polys_batch"], r_z)
    if final is None or final != sum(pow(rho, k, q) * _eq_at(x, r_z) % q * e for k, (x, e) in enumerate(zip(points, proof["evals_batch"]))) % q:
        return rej(BATCH)
    tr.absorb_scalars(b"evals_batch", list(proof["evals_batch"]))
    gamma = tr.squeeze(b"gamma", q)
    comm_joint, y = None, 0
    for k, (cm, e) in enumerate(zip(comms, proof["evals_batch"])):
        comm_joint = CURVE.add(comm_joint, CURVE.mul(pow(gamma, k, q), cm))
        y = (y + pow(gamma, k, q) * e) % q
    return _check_opening(tr, ell, comm_joint, y, r_z, proof)


def make_instance(tau: int, num_cons: int, num_vars: int, nio: int, seed: int, folded: bool) -> dict:
    mats, X, u, W, E = product_instance(num_cons, num_vars, nio, seed, folded)
    return dict(mats=mats, num_cons=num_cons, num_vars=num_vars, X=X, u=u, W=W, E=E, comm_W=commit(tau, W), comm_E=commit(tau, E))
