"""A plain reference for the user side of a score -- MVIN._key_addressing (model.py:161-240) and the user MLP of :232-236 -- and the inputs
that put its softmaxes where a trained model puts them.  Written from the reference's formulas with plain torch indexing; nothing here is
shared with the code under test.

keyaddr_reference(..., dtype=torch.float64) is the reference; dtype=torch.float32 evaluates the same formulas op by op in fp32 and is the
YARDSTICK: err_f32 of an output = the largest max |fp32 - float64| over the evaluation orders the kernels use,
    "vr_h":  V = E[item] . R_KGE[r], logit = V . E[h]          (mvin_key_addressing_fwd's contract: the caller forms V)
    "rh_v":  U = R_KGE[r] . E[h],    logit = U . E[item]       (the grouped kernels and the flash form's per-call table)
and, for user_o only and only where asked (tw=True: the flash form), the user MLP applied per entity before the weighted sum,
    user_o = sum_m p_m (E[t_m] . W_j) + b   (mvin_key_addressing_flash_prepare's TW tables)   next to   (sum_m p_m E[t_m]) . W_j + b.
It is taken over at least YARDSTICK_PAIRS pairs drawn like the case's own, of which the case's pairs are the first B (the maximum over a
handful of draws is no yardstick: tests/test_gpu_fold_f64.py's docstring has the figures).

build_inputs(regime, ...) draws the tables, ripple sets and pairs of one logit regime and condition(inp, ref64) asserts, in float64 on the
reference's own logits, that the regime is what it claims -- for ALL rows, so that an input that silently degenerates fails the test that uses it:
    unit        today's inputs, the control: for the per-pair feeds E = 0.5 N(0,1), R_KGE = N(0,1)/sqrt(D), w = N(0,1) (test_gpu_keyaddr.py, logit
                sd about 2), for pairs grouped by user everything uniform in +-0.5 (test_gpu_user_records.py, logit sd about 1.5).
    sharp       E = 2 c N(0,1), R_KGE = N(0,1)/sqrt(D), w = 2 c N(0,1), c = (64/D)^(1/4): logit sd about 32 at every D.  Entity rows are
                rescaled to their expected length 2 c sqrt(D) (at D = 16 one item in a few hundred is short enough to halve its rows'
                logits otherwise).  Every row of at least 32 memories spreads (max - min) by 60 or more; over rows of fewer memories (a
                row of ONE memory has no spread, a row of five draws spreads by less than 60 now and then) the logits' standard
                deviation is at least 20.
The other four share one structure: E[e] = s (g_e u0 + n_e) with u0 a unit vector and n_e a small noise orthogonal to it,
R_KGE[r] = a_r I + small noise, w = s u0, so that a hop logit is s^2 a_r g_item g_h (+ noise) and an h-set logit s^2 g_h, whatever the item.
    planted     one entity S with g = 60 among g = 1, a in [0.8, 1.2]: the memory whose head is S wins its row outright (hop gap >= 40).
                Its slot walks over the row as the user index increases, the slots where kernels change path first: 0, the last row of a
                16-row tile, the first of the next, the last valid row before the padding rows; hop j starts ceil(Nm / P) slots further.
                Tails are distinct within a row, so the o-vector names the slot: it equals E[t*] to a few ulp.
    ascending   g_h linear in the slot from 1 to 2 and the row's relations sorted by a_r, s^2 chosen from Nm: the running maximum over
                the memory index rises by 1 or more (about 4 by construction) across every 16-row boundary of every row -- every online
                rescale and every merge of parts happens with a factor far from 1.
    descending  the same rows reversed: slot 0 holds the maximum of every row, no rescale is ever taken after it.
    offset      g = 10 for every entity, a_r = 1 +- 0.005, noise NOT orthogonal: every logit near +100 (all above 88, where expf overflows
                fp32), mean row spread below 5.  A softmax that forgot its maximum overflows here."""
import types

import numpy as np
import torch

YARDSTICK_PAIRS = 256
REGIMES = ["unit", "sharp", "planted", "ascending", "descending", "offset"]


def _lists(mem, users):
    """(mh, mr, mt) per-hop lists of [B, Nm] long tensors from either feed: uts [n_user, P, 3, Nm] + users, or the lists themselves."""
    if isinstance(mem, (tuple, list)):
        return tuple([t.long() for t in lst] for lst in mem)
    sel = mem[users.long()].long()                            # [B, P, 3, Nm]
    return tuple([sel[:, j, x] for j in range(sel.shape[1])] for x in range(3))


def keyaddr_reference(E, R_KGE, w, W_mlp, b_mlp, mem, users, items, P, dtype=torch.float64, order="rh_v", tw=False):
    """model.py:161-240 for the pairs (users[b], items[b]).  E [n_entity, D] holds the values the kernel reads (a bf16 table: its rows widened
    to fp32); ``mem`` = user_triplet_set [n_user, max(1, P), 3, Nm] (pair b reads users[b]'s sets) or the per-pair lists (mh, mr, mt).
    -> o [B, (w is not None) + P, D], user_o [B, D] (None without W_mlp), logits, probs (lists of [B, Nm], one per o-vector).
    The h-set logit is E[h] . w: the user term and the bias of :171 are constant over the memories and cancel in the softmax."""
    f = lambda t: t.to(dtype)                                 # noqa: E731
    Ed, Rd = f(E), (f(R_KGE) if R_KGE is not None else None)
    mh, mr, mt = _lists(mem, users)
    v = Ed[items.long()]                                      # [B, D]
    o, logits, probs = [], [], []
    if w is not None:
        h = Ed[mh[0]]                                         # [B, Nm, D]
        s = h @ f(w)                                          # :171 without the terms constant over m
        p = torch.softmax(s, dim=-1)                          # :189
        o.append((p[..., None] * h).sum(1))                   # :195
        logits.append(s), probs.append(p)
    if P > 0:
        if order == "vr_h":
            V = torch.einsum("bi,rij->brj", v, Rd)            # V[b, r, :] = E[item_b] . R_KGE[r]
        else:
            U = torch.einsum("rij,ej->rei", Rd, Ed)           # U[r, e, :] = R_KGE[r] . E[e]      (:214-217)
    for hop in range(P):
        if order == "vr_h":
            Vm = torch.gather(V, 1, mr[hop][..., None].expand(-1, -1, V.shape[-1]))     # [B, Nm, D]
            s = (Vm * Ed[mh[hop]]).sum(-1)
        else:
            s = (U[mr[hop], mh[hop]] * v[:, None, :]).sum(-1)                           # :220
        p = torch.softmax(s, dim=-1)                          # :223
        o.append((p[..., None] * Ed[mt[hop]]).sum(1))         # :229
        logits.append(s), probs.append(p)
    o = torch.stack(o, 1)
    user_o = None
    if W_mlp is not None:
        D = Ed.shape[1]
        if tw:                                                # the MLP per entity first, then the weighted sum
            user_o = f(b_mlp).expand(o.shape[0], -1).clone()
            vals = ([mh[0]] if w is not None else []) + list(mt[:P])
            for j, (ids, p) in enumerate(zip(vals, probs)):
                TW = Ed @ f(W_mlp[j * D:(j + 1) * D])
                user_o = user_o + (p[..., None] * TW[ids]).sum(1)
        else:
            user_o = o.reshape(o.shape[0], -1) @ f(W_mlp) + f(b_mlp)                    # :232-236
    return types.SimpleNamespace(o=o, user_o=user_o, logits=logits, probs=probs)


def yardstick(inp, ref64, tw=False):
    """err_f32 per output over ALL of ``inp``'s pairs: {"o": ..., "user_o": ...}, the larger of the evaluation orders' max |fp32 - float64|."""
    err = {"o": 0.0, "user_o": 0.0}
    for order in ("vr_h", "rh_v"):
        for t in ((False, True) if tw else (False,)):
            r32 = reference(inp, torch.float32, order=order, tw=t)
            if not t:
                err["o"] = max(err["o"], float((r32.o.double() - ref64.o).abs().max()))
            err["user_o"] = max(err["user_o"], float((r32.user_o.double() - ref64.user_o).abs().max()))
    return err


def reference(inp, dtype=torch.float64, order="rh_v", tw=False, n=None):
    """keyaddr_reference on the first ``n`` pairs (all of them when None) of build_inputs' result."""
    n = inp.users.shape[0] if n is None else n
    return keyaddr_reference(inp.E, inp.R, inp.w, inp.W_mlp, inp.b_mlp, inp.uts, inp.users[:n], inp.items[:n], inp.P, dtype, order, tw)


def key_slots(Nm):
    """Every slot of a row, the ones where a kernel changes path first: row 0, the last valid row, the last row of every 16-row tile and the
    first of the next."""
    first = [0, Nm - 1]
    for b in range(16, Nm, 16):
        first += [b - 1, b]
    seen, order = set(), []
    for m in first + list(range(Nm)):
        if 0 <= m < Nm and m not in seen:
            seen.add(m)
            order.append(m)
    return order


def planted_slot(u, hop, P, Nm):
    return key_slots(Nm)[(u + hop * (-(-Nm // max(1, P)))) % Nm]


def ascending_scale(Nm):
    """s^2 of the ascending / descending rows: the last 16-row boundary is followed by n_last rows, which must lift the running maximum by about 4
    at the smallest item and relation coefficients (g = 1, a = 0.8): 0.8 s^2 n_last / (Nm - 1) >= 4."""
    n_last = Nm - 16 * ((Nm - 1) // 16)
    return max(25.0, 5.0 * (Nm - 1) / n_last)


def build_inputs(regime, D, Nm, P, nR, n_pairs, n_user=None, n_entity=700, has_set=True, bf16=False, seed=0, device="cpu"):
    """Tables, ripple sets and max(n_pairs, YARDSTICK_PAIRS) pairs of one regime; the case's own pairs are the first n_pairs.  ``n_user`` None:
    one user per pair (the per-pair feeds: users = 0, 1, 2, ...); else pairs drawn over n_user users.  bf16: E holds bf16-rounded values
    (inp.E_table is the bf16 tensor the kernel takes).  Everything fp32 on ``device``; ids int32 (uts) / int64 (users, items)."""
    assert regime in REGIMES
    rng = np.random.default_rng([REGIMES.index(regime), D, Nm, P, nR, seed])
    N = max(n_pairs, YARDSTICK_PAIRS)
    Ph = max(1, P)
    nU = N if n_user is None else n_user
    users = np.arange(N) if n_user is None else rng.integers(0, n_user, N)
    uts = np.empty((nU, Ph, 3, Nm), dtype=np.int32)
    uts[:, :, 0] = rng.integers(0, n_entity, (nU, Ph, Nm))
    uts[:, :, 1] = rng.integers(0, nR, (nU, Ph, Nm))
    uts[:, :, 2] = rng.integers(0, n_entity, (nU, Ph, Nm))
    items = rng.integers(0, n_entity, N)
    normal = lambda *s: rng.normal(size=s)                    # noqa: E731
    special = None
    W_mlp = b_mlp = None
    n_o = P + (1 if has_set else 0)
    if regime == "unit" and n_user is None:                   # test_gpu_keyaddr.py's draws
        E, R, w = 0.5 * normal(n_entity, D), normal(nR, D, D) / np.sqrt(D), normal(D)
    elif regime == "unit":                                    # test_gpu_user_records.py's / test_gpu_flash.py's draws
        uniform = lambda *s: rng.random(s) - 0.5              # noqa: E731
        E, R, w = uniform(n_entity, D), uniform(nR, D, D), uniform(D)
        W_mlp, b_mlp = 0.3 * uniform(n_o * D, D), uniform(D)
    elif regime == "sharp":
        c = (64.0 / D) ** 0.25
        E, R, w = 2 * c * normal(n_entity, D), normal(nR, D, D) / np.sqrt(D), 2 * c * normal(D)
        E *= np.sqrt(D) / np.linalg.norm(E / (2 * c), axis=1, keepdims=True)      # every row at its expected length
    else:
        u0 = normal(D)
        u0 /= np.linalg.norm(u0)
        noise = normal(n_entity, D)
        a = rng.uniform(0.8, 1.2, nR)
        s2 = 1.0
        if regime == "offset":
            g = np.full(n_entity, 10.0)
            noise *= 0.05                                     # not orthogonal to u0: 10 u0 . n_e is the row's spread (sd 0.5)
            a = 1.0 + 0.005 * normal(nR)
        else:
            noise = (noise - np.outer(noise @ u0, u0)) * (0.1 / np.sqrt(D))
            if regime == "planted":
                g = np.ones(n_entity)
                special = int(rng.integers(0, n_entity))
                g[special] = 60.0
            else:
                g = 1.0 + np.arange(n_entity) / (n_entity - 1.0)
                s2 = ascending_scale(Nm)
        s = np.sqrt(s2)
        E = s * (g[:, None] * u0[None, :] + noise)
        R = a[:, None, None] * np.eye(D)[None] + normal(nR, D, D) * (0.01 / np.sqrt(D))
        w = (10.0 if regime == "offset" else s) * u0         # h-set logits on the hops' scale
        for u in range(nU):                                   # tails distinct within a row: the output names the slot
            for j in range(Ph):
                uts[u, j, 2] = rng.choice(n_entity, Nm, replace=Nm > n_entity)
        if regime == "planted":
            heads = uts[:, :, 0]
            heads[heads == special] = (special + 1) % n_entity
            items[items == special] = (special + 1) % n_entity
            for u in range(nU):
                for j in range(Ph):
                    uts[u, j, 0, planted_slot(u, j, P, Nm)] = special
        elif regime in ("ascending", "descending"):
            a_eff = np.einsum("i,rij,j->r", u0, R.astype(np.float32).astype(np.float64), u0)      # the coefficient R_KGE[r] really carries
            tgt = 1.0 + np.arange(Nm) / max(1, Nm - 1)        # g_h of slot m
            head = np.rint((tgt - 1.0) * (n_entity - 1)).astype(np.int32)
            for u in range(nU):
                for j in range(Ph):
                    r = uts[u, j, 1]
                    r = r[np.argsort(a_eff[r], kind="stable")]
                    uts[u, j, 0], uts[u, j, 1] = head, r
            if regime == "descending":
                uts = uts[..., ::-1].copy()
    if W_mlp is None:
        W_mlp, b_mlp = 0.1 * normal(n_o * D, D), 0.1 * normal(D)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)       # noqa: E731
    inp = types.SimpleNamespace(regime=regime, D=D, Nm=Nm, P=P, nR=nR, n_entity=n_entity, n_user=nU, n_pairs=n_pairs, has_set=has_set,
                                special=special, bf16=bf16)
    inp.E_table = t(E).to(torch.bfloat16) if bf16 else t(E)
    inp.E = inp.E_table.float()                               # the values the kernel reads
    inp.R, inp.w, inp.W_mlp, inp.b_mlp = t(R), (t(w) if has_set else None), t(W_mlp), t(b_mlp)
    inp.uts = torch.from_numpy(uts).to(device)
    inp.users, inp.items = torch.from_numpy(users.astype(np.int64)).to(device), torch.from_numpy(items.astype(np.int64)).to(device)
    return inp


def planted_rows(inp, n=None):
    """-> (slots [n, n_o] long, tails [n, n_o, D]): the planted slot of every o-vector of the first n pairs and the row E[t*] it must return
    (the h-set read returns the head itself)."""
    n = inp.users.shape[0] if n is None else n
    u = inp.users[:n].cpu().numpy()
    blocks = ([(0, 0)] if inp.has_set else []) + [(j, 2) for j in range(inp.P)]
    slots = np.array([[planted_slot(int(x), j, inp.P, inp.Nm) for (j, _) in blocks] for x in u])
    sel = inp.uts[inp.users[:n].long()].long()                # [n, P, 3, Nm]
    st = torch.from_numpy(slots).to(sel.device)
    ids = torch.stack([sel[torch.arange(n), j, x, st[:, k]] for k, (j, x) in enumerate(blocks)], 1)
    return st, inp.E[ids]


def condition(inp, ref64):
    """Assert, in float64 on the reference's logits, that ``inp`` is the regime it claims, for every row of every pair (the yardstick's pairs
    included)."""
    Nm, regime = inp.Nm, inp.regime
    L = torch.stack(ref64.logits, 1).double()                 # [N, n_o, Nm]
    assert torch.isfinite(L).all()
    spread = L.max(-1).values - L.min(-1).values
    if regime == "unit":
        assert float(L.abs().max()) < 40
    elif regime == "sharp":
        if Nm >= 32:
            assert float(spread.min()) >= 60, f"sharp: a row spreads by {float(spread.min()):.1f} only"
        elif Nm >= 2:
            assert float(L.std()) >= 20, f"sharp: logit sd {float(L.std()):.1f}"
    elif regime == "planted":
        slots, _ = planted_rows(inp)
        assert torch.equal(L.argmax(-1), slots.to(L.device)), "planted: the argmax is not the planted slot"
        if Nm >= 2:
            top = L.topk(2, dim=-1).values
            gap = float((top[..., 0] - top[..., 1]).min())
            assert gap >= 40, f"planted: the winner leads by {gap:.1f} only"
    elif regime in ("ascending", "descending"):
        if regime == "ascending":
            run = torch.cummax(L, dim=-1).values
            for b in range(16, Nm, 16):                       # the running maximum after the tile that starts at b against the one before it
                rise = float((run[..., min(b + 16, Nm) - 1] - run[..., b - 1]).min())
                assert rise >= 1, f"ascending: the running maximum rises by {rise:.2f} only across row {b}"
        else:
            assert bool((L.argmax(-1) == 0).all()), "descending: slot 0 does not hold the maximum"
            if Nm > 16:
                lead = float((L[..., 0] - L[..., 16:].max(-1).values).min())
                assert lead >= 1, f"descending: slot 0 leads the later tiles by {lead:.2f} only"
    elif regime == "offset":
        assert float(L.min()) > 88, f"offset: a logit of {float(L.min()):.1f}"
        if Nm >= 2:
            assert float(spread.mean()) < 5, f"offset: mean spread {float(spread.mean()):.2f}"


def _c(D, Nm, P, nR, B, n_user=None, has_set=True, bf16=False):
    return dict(D=D, Nm=Nm, P=P, nR=nR, n_pairs=B, n_user=n_user, has_set=has_set, bf16=bf16)


# The shapes of tests/test_gpu_keyaddr_sharp.py, form by form (tests/test_keyaddr_ref_host.py checks every regime's condition at each of them on the CPU)
CASES = {
    # mvin_keyaddr_stream.hip: the largest V block it takes, one memory / one over a tile / padding rows / four full tiles
    "stream": [_c(D, Nm, 2, 3072 // (4 * D), 37, bf16=bf) for bf in (False, True) for D in (16, 32, 64, 128) for Nm in (1, 17, 40, 64)
               if not (bf and D == 16)],                      # bf16 rows of 32 bytes: not a table shape the library takes
    "register": [_c(64, 16, 1, 39, 33), _c(32, 100, 2, 12, 33)],
    "users_feed": [_c(64, 64, 2, 9, 301, n_user=37)],
    "general": [_c(64, 300, 1, 9, 29), _c(32, 5, 1, 9, 29)],  # one hop: mode 1 is its h-set read, mode 0 its hop
    "wave": [_c(16, 64, 2, 9, 300, 30), _c(32, 40, 2, 12, 300, 30), _c(16, 1, 1, 5, 300, 30)],
    "dense": [_c(64, 40, 2, 9, 300, 30), _c(64, 48, 3, 9, 300, 30, has_set=False), _c(64, 80, 2, 9, 300, 30), _c(64, 64, 2, 9, 300, 30, bf16=True),
              _c(128, 16, 1, 7, 300, 30), _c(64, 64, 2, 9, 1500, 700)],
    "static": [_c(64, 64, 2, 9, 300, 30), _c(64, 40, 2, 9, 300, 30), _c(64, 32, 4, 7, 300, 30), _c(64, 64, 2, 25, 300, 30)],
    "er": [_c(64, 64, 2, 9, 300, 30), _c(64, 40, 2, 9, 300, 30)],
    "flash": [_c(64, 64, 2, 9, 300, 30), _c(64, 40, 2, 9, 300, 30), _c(64, 16, 1, 39, 300, 30), _c(64, 8, 8, 5, 300, 30), _c(64, 1, 2, 1, 300, 30)],
}


def case_id(c):
    return "D%dNm%dP%dnR%d_B%d%s%s%s" % (c["D"], c["Nm"], c["P"], c["nR"], c["n_pairs"], "" if c["n_user"] is None else "_u%d" % c["n_user"],
                                         "" if c["has_set"] else "_noset", "_bf16" if c["bf16"] else "")
