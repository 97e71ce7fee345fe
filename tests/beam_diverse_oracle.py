"""Test infrastructure: the diverse (group) beam-search pick (include/set_hip.h set_beam_pick_diverse_f32) restated in float64
numpy over the FULL g V candidates of every group, and the search around it.  The k slots of an image are G groups of g = k / G;
group gi picks by the key y = x - penalty n(word), n = the counted non-<end> picks of groups 0 .. gi - 1 of this step with that
word, and carries x.  Candidate values, the three removal rules and the rank score are tests/beam_constrained_oracle.py's.
`rows_only=True` is the variant the kernel implements — every row offers only its k best survivors — which the lemma of
tests/test_beam_diverse_cpu.py proves equal."""
import numpy as np

import beam_constrained_oracle as BO

NONE = BO.NONE


def new_state(NI, k, G, Lmax, start, dtype=np.float64):
    """the state at the start of a search: only the first slot of every group is alive"""
    g = k // G
    st = BO.new_state(NI, k, Lmax, start, dtype)
    st["scores"][:] = -np.inf
    st["scores"][:, ::g] = 0.0
    st["g_left"] = np.full((NI, G), g, np.int32)
    st["done_group"] = np.zeros((NI, k), np.int32)
    return st


def row_values(st, lp, i, k, V, L, c, end, rows_only):
    """(k, V) candidate values of image i from the state before the step: -inf for a dead slot and for a removed word"""
    X = np.full((k, V), -np.inf)
    for j in range(k):
        sc = st["scores"][i, j]
        if sc == -np.inf:
            continue
        x = (sc + lp[i * k + j]).copy()
        x[[w for w in BO.removed_words(st["seqs"][i, j, :L], c, end) if 0 <= w < V]] = -np.inf
        x[np.isnan(x)] = -np.inf
        if rows_only:                                                     # value descending, word ascending: the row's k best
            keep = np.lexsort((np.arange(V), -x))[:k]
            y = np.full(V, -np.inf)
            y[keep] = x[keep]
            x = y
        X[j] = x
    return X


def pick(logits, logits2, st, cur_len, c, k, V, end, G, penalty, rows_only=False):
    """One step, in place on st (new_state's arrays, float64 floats).  logits (NI * k, >= V).  -> (seqs_out, words, rows, info);
    info[i] = None for an image that was finished before the step, else a list of G entries: None for a group that had ended, else
      top      the g + 1 best (key y, flat j V + v, value x) of the group (fewer if there are fewer finite ones)
      counted  how many picks counted, exhausted = the group ended for want of a survivor"""
    NI = st["scores"].shape[0]
    g, L = k // G, cur_len
    lp = BO.logp64(np.asarray(logits)[:, :V], None if logits2 is None else np.asarray(logits2)[:, :V])
    words, rows = np.zeros(NI * k, np.int64), np.zeros(NI * k, np.int32)
    out = st["seqs"].copy()
    info = []
    for i in range(NI):
        if int(st["k_left"][i]) <= 0:
            rows[i * k:(i + 1) * k] = np.arange(i * k, (i + 1) * k)
            info.append(None)
            continue
        X = row_values(st, lp, i, k, V, L, c, end, rows_only)
        seqs_in = st["seqs"][i].copy()
        n = np.zeros(V)                                                   # n(v) so far
        ginfo = []
        for gi in range(G):
            lo = gi * g
            gl = int(st["g_left"][i, gi])
            if gl <= 0:
                rows[i * k + lo:i * k + lo + g] = np.arange(i * k + lo, i * k + lo + g)
                ginfo.append(None)
                continue
            x = X[lo:lo + g].reshape(-1)
            with np.errstate(invalid="ignore"):
                y = x - penalty * np.tile(n, g)
            y[x == -np.inf] = -np.inf
            top = [(float(y[f]), int(f) + lo * V, float(x[f])) for f in BO._best(y, g + 1) if y[f] > -np.inf]
            inf_g = dict(top=top, counted=0, exhausted=not top)
            ginfo.append(inf_g)
            if not top:                                                   # exhausted: the group ends here
                st["g_left"][i, gi] = 0
                st["scores"][i, lo:lo + g] = -np.inf
                rows[i * k + lo:i * k + lo + g] = np.arange(i * k + lo, i * k + lo + g)
                continue
            picks = [(top[r][2], top[r][1]) if r < min(len(top), g) else (-np.inf, NONE) for r in range(g)]
            ok = [flat != NONE and r < gl for r, (v, flat) in enumerate(picks)]
            inf_g["counted"] = sum(ok)
            ends = [r for r, (v, flat) in enumerate(picks) if ok[r] and flat % V == end]
            rs = {r: BO.rank_score(picks[r][0], L, c.length_alpha) for r in ends}
            if ends:
                r0 = max(ends, key=lambda r: (rs[r], -r))                # first maximum
                if rs[r0] > st["best_score"][i]:
                    st["best_score"][i], st["best_len"][i] = rs[r0], L + 1
                    st["best_seq"][i, :L] = seqs_in[picks[r0][1] // V, :L]
                    st["best_seq"][i, L] = end
            for r in ends:
                at = int(st["n_done"][i])
                if at >= k:
                    continue
                st["done_score"][i, at], st["done_len"][i, at], st["done_group"][i, at] = rs[r], L + 1, gi
                st["done_seq"][i, at, :L] = seqs_in[picks[r][1] // V, :L]
                st["done_seq"][i, at, L] = end
                st["n_done"][i] += 1
            st["g_left"][i, gi] = gl - len(ends)
            live = [r for r in range(g) if ok[r] and r not in ends]
            for slot, r in enumerate(live + [r for r in range(g) if r not in live]):
                v, flat = picks[r]
                parent, word = (flat // V, flat % V) if flat != NONE else (lo, 0)
                assert lo <= parent < lo + g                              # a parent and its child are in one group
                st["scores"][i, lo + slot] = v if r in live else -np.inf
                words[i * k + lo + slot] = word if r in live else 0
                rows[i * k + lo + slot] = i * k + parent
                out[i, lo + slot, :L] = seqs_in[parent, :L]
                out[i, lo + slot, L] = word
                if r in live:
                    n[word] += 1
        st["k_left"][i] = int(st["g_left"][i].sum())
        info.append(ginfo)
    return out, words, rows, info


def groups_of(info):
    """every (image, group, entry) of one step's info that picked or ran out"""
    return [(i, gi, e) for i, gs in enumerate(info) if gs for gi, e in enumerate(gs) if e]


def min_gap(info):
    """the smallest difference between adjacent keys among the g + 1 best of any group of one step"""
    gap = np.inf
    for _, _, e in groups_of(info):
        v = [y for y, _, _ in e["top"]]
        gap = min([gap] + [a - b for a, b in zip(v, v[1:])])
    return gap


def group_answers(st, i, k, G, start, length):
    """image i -> (the G (tokens, score) in group order, every completed (tokens, score, group) by score descending, equal scores
    in completion order).  A group's answer: its best completed hypothesis by rank score (first maximum); (its first slot's
    `length` tokens, nan) when it is still alive with nothing completed; ([start], nan) when it ran out of candidates"""
    g = k // G
    done = [(st["done_seq"][i, j, :st["done_len"][i, j]].tolist(), float(st["done_score"][i, j]), int(st["done_group"][i, j]))
            for j in range(int(st["n_done"][i]))]
    ans = []
    for gi in range(G):
        mine = [e for e in done if e[2] == gi]
        if mine:
            best = max(range(len(mine)), key=lambda q: (mine[q][1], -q))
            ans.append((mine[best][0], mine[best][1]))
        elif st["g_left"][i, gi] > 0:
            ans.append((st["seqs"][i, gi * g, :length].tolist(), float("nan")))
        else:
            ans.append(([start], float("nan")))
    return ans, sorted(done, key=lambda e: -e[1])


def search(step, reindex, NI, k, V, start, end, c, max_steps, G, penalty):
    """evaluate.beam_search_diverse on the oracle's pick.  step(words (NI * k)) -> list of one or two (NI * k, V) logits;
    reindex(rows (NI * k)) re-indexes the models' state.  -> (answers, completed, steps): group_answers of every image and the
    info of every pick."""
    Lmax = max_steps + 2
    st = new_state(NI, k, G, Lmax, start)
    words = np.full(NI * k, start, np.int64)
    steps = []
    cur = 0
    for cur in range(1, max_steps + 2):
        lg = step(words)
        out, words, rows, info = pick(lg[0], lg[1] if len(lg) > 1 else None, st, cur, c, k, V, end, G, penalty)
        st["seqs"] = out
        reindex(rows)
        steps.append(info)
        if int(st["k_left"].max()) == 0:
            break
    res = [group_answers(st, i, k, G, start, cur + 1) for i in range(NI)]
    return [r[0] for r in res], [r[1] for r in res], steps
