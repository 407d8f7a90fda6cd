"""Genotype-free demultiplexing: EM clustering of barcodes into K donors from the reads alone, then doublet calls between the clusters.

The model is a mixture of K donors whose genotypes are unknown.  Each restart r of R runs its own EM over K columns of one engine of
V = R * K columns:
  E-step   K1 (Engine.run_singlet) scores every barcode against every column of the current cluster genotypes; cluster_estep turns
           llks + log pi into per-(barcode, column) weights on the device and returns the per-restart log-likelihood and column sums.
  M-step   cluster_mstep pools the per-pair log genotype likelihoods with those weights into a posterior gp' = (q + floor) x likelihood,
           q the per-SNP Hardy-Weinberg prior from the pooled allele counts; gp' stays on the device and becomes K1's matrix.
The restart with the highest log-likelihood gives the K genotype columns (sample ids CLUST0 .. CLUST{K-1}); the unchanged
`demuxlet_run` writes <prefix>.best/.single/.sing2 from them (doublets come out of its grid), and each round r >= 1 refines the
clusters' genotypes from the previous round's singlets only (the refinement of section 12, prior q) and runs again to <prefix>.r<r>.*.
With em_doublets (--em-doublets) each restart also has a doublet component for every pair of its clusters, a
50/50 mixture (alpha = 0.5) with prior share delta_r: cluster_doublet scores them after K1, cluster_estep_doublet gives the singlet
weights (a doublet's mass goes to no cluster) and the doublet mass from which delta_r is re-estimated.

With split_merge (--split-merge) the winning restart then goes through split-merge moves: merge scores of every
pair of its clusters (cluster_merge_score), a 2-component sub-EM inside every cluster (cluster_estep_grouped), and candidate restarts
that merge one pair and split one cluster into the freed column; the best candidate replaces the winner when its converged LL is higher.

With auto_k (--auto-k) n_clusters is an upper bound K_max: after the EM at K_max every restart walks a merge path
down to k_min clusters.  Each state is turned into hard labels on the device (cluster_hard), an M-step on their one-hot matrix gives the
pooled genotype likelihoods, and the state's score is the model evidence of those labels (cluster_evidence, path_score); the pair of
highest merge score (cluster_merge_score) is then merged (cluster_merge_columns), its column goes inactive (log pi = -inf) and the EM
converges again.  The (state, restart) of highest score gives K and the genotype columns; <prefix>.kpath.tsv records the path.

    python -m demuxlet_amd.cluster --pileup <x>.pileup.txt --n-clusters K --out <prefix> [--restarts R] [--seed S] [--max-iter N]
        [--tol T] [--floor F] [--min-snp M] [--alpha A ...] [--rounds N] [--match] [--em-doublets] [--split-merge] [--auto-k [--k-min M]]
        [--fast] [--gpu G]

reads the dump that `demuxlet --pileup-only` writes; its genotype matrix is ignored unless --match is given."""
from __future__ import annotations

import argparse
import sys
from math import lgamma
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import capi, engine, refine

MAX_COLUMNS = 4094          # dmx_engine_create's widest panel: R * K columns in one engine
# Restarts: EM from a random hard assignment often settles where one cluster holds two donors and another donor is split.  The true
# solution's log-likelihood is clearly higher, so more restarts help; measured on synthetic pools of 4 000 barcodes x ~1 000 covered
# SNPs (tests/test_gpu_cluster.py): 3 of 6 single restarts found the donors at K = 4, 0 of 6 at K = 8; the best of 16 did at both.
PI_FLOOR = 1e-6             # smallest mixing weight a cluster keeps between iterations
EM_HEADER = "ITER\tRESTART\tLLK\tPI\n"
EM_HEADER_DBL = "ITER\tRESTART\tLLK\tPI\tDBL\n"
# doublet-aware EM: each restart's doublet share delta starts at DELTA0 and is re-estimated after every E-step, clipped to
# [DELTA_MIN, DELTA_MAX] (a share above one half would let the doublet components absorb a cluster)
DELTA0, DELTA_MIN, DELTA_MAX = 0.1, 1e-3, 0.5
MATCH_HEADER = "CLUST\tSM_ID\tN.CELL\tSUM.LLK\tBEST\n"
# split-merge moves: the top A merges x top S splits are the candidates of a move, each split by the best of Rs random-half sub-restarts
SM_CANDIDATES = (3, 3)
SM_SPLIT_RESTARTS = 4
SM_MAX_K = 64               # dmx_engine_cluster_merge_score stages K columns per SNP in LDS
AUTO_K_MAX = SM_MAX_K         # the merge path scores pairs with dmx_engine_cluster_merge_score
KPATH_HEADER = "STEP\tRESTART\tK\tLLK\tSCORE\tEVIDENCE\tDBL.SCORE\tLABEL.TERM\tN.SNG\tN.DBL\tSIZES\tMERGE_K\tMERGE_L\tBF\tCHOSEN\n"
MOVES_HEADER = "MOVE\tCAND\tMERGE_K\tMERGE_L\tSPLIT\tBF\tSPLIT_GAIN\tLLK_BEFORE\tLLK_AFTER\tITER\tACCEPTED\n"


def cluster_ids(k: int) -> List[str]:
    return [f"CLUST{j}" for j in range(k)]


def check_args(n_clusters: int, restarts: int, max_iter: int, tol: float, floor: float, n_cells: int, n_pairs: int) -> None:
    """The error paths of cluster_run, before any device work."""
    if n_clusters < 2:
        raise ValueError(f"--n-clusters {n_clusters}: clustering needs at least 2 clusters")
    if restarts < 1:
        raise ValueError(f"--restarts {restarts}: at least 1")
    if n_clusters * restarts > MAX_COLUMNS:
        raise ValueError(f"{restarts} restarts x {n_clusters} clusters = {n_clusters * restarts} columns; one engine holds at most {MAX_COLUMNS}")
    if max_iter < 1:
        raise ValueError(f"--max-iter {max_iter}: at least 1")
    if not (tol >= 0.0) or not (floor >= 0.0):
        raise ValueError("--tol and --floor must be >= 0")
    if n_cells < n_clusters or n_pairs == 0:
        raise ValueError(f"empty pileup: {n_cells} barcodes, {n_pairs} covered (barcode, SNP) pairs for {n_clusters} clusters")


def check_sm_args(n_clusters: int, candidates: Sequence[int], split_restarts: int, max_moves: Optional[int]) -> None:
    """The error paths of split_merge=True, before any device work."""
    a, b = (int(x) for x in candidates)
    if n_clusters > SM_MAX_K:
        raise ValueError(f"split-merge moves support at most {SM_MAX_K} clusters, not {n_clusters}")
    if a < 1 or b < 1 or split_restarts < 1:
        raise ValueError("--sm-candidates and --sm-split-restarts must be >= 1")
    if a * b * n_clusters > MAX_COLUMNS or 2 * split_restarts * n_clusters > MAX_COLUMNS:
        raise ValueError(f"{a} x {b} candidates or {split_restarts} split restarts of {n_clusters} clusters exceed {MAX_COLUMNS} columns")
    if max_moves is not None and max_moves < 0:
        raise ValueError(f"--sm-max-moves {max_moves}: at least 0")


def check_auto_k_args(n_clusters: int, k_min: int, split_merge: bool) -> None:
    """The error paths of auto_k=True, before any device work: 2 <= k_min <= K_max <= AUTO_K_MAX, and no split-merge moves."""
    if split_merge:
        raise ValueError("--auto-k and --split-merge do not go together (run split-merge at the chosen K afterwards, from init_labels)")
    if n_clusters > AUTO_K_MAX:
        raise ValueError(f"--auto-k walks down from at most {AUTO_K_MAX} clusters, not {n_clusters}")
    if k_min < 2 or k_min > n_clusters:
        raise ValueError(f"--k-min {k_min}: must be in [2, --n-clusters {n_clusters}]")


def check_init_labels(labels, n_cells: int, n_clusters: int) -> np.ndarray:
    """init_labels as int32 [R][B] with every entry in [-1, K) (-1: the barcode takes no part in the first M-step)."""
    lab = np.asarray(labels)
    if lab.ndim == 1:
        lab = lab[None, :]
    if lab.ndim != 2 or lab.shape[1] != n_cells or lab.shape[0] < 1:
        raise ValueError(f"init_labels must be [R][{n_cells}], not {lab.shape}")
    if not np.issubdtype(lab.dtype, np.integer):
        raise ValueError("init_labels must be integers")
    if lab.size and (lab.min() < -1 or lab.max() >= n_clusters):
        raise ValueError(f"init_labels must be in [-1, {n_clusters})")
    return np.ascontiguousarray(lab, dtype=np.int32)


def hwe_prior(n_ref: np.ndarray, n_alt: np.ndarray) -> np.ndarray:
    """q[S][3] float32 = Hardy-Weinberg genotype frequencies of p = (n_alt + 1) / (n_ref + n_alt + 2), the pooled ALT frequency."""
    p = (np.asarray(n_alt, dtype=np.float64) + 1.0) / (np.asarray(n_ref, dtype=np.float64) + np.asarray(n_alt, dtype=np.float64) + 2.0)
    return np.stack([(1.0 - p) ** 2, 2.0 * p * (1.0 - p), p * p], axis=1).astype(np.float32)


def initial_labels(seed: int, restarts: int, n_cells: int, n_clusters: int) -> np.ndarray:
    """labels[R][B]: each restart's random hard assignment, from one seeded numpy Generator."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, n_clusters, size=n_cells) for _ in range(restarts)]).astype(np.int32)


def one_hot_weights(labels: np.ndarray, n_clusters: int, mask: Optional[np.ndarray] = None) -> np.ndarray:
    """w[B][R * K] float64: 1 at column r * K + labels[r][b], 0 elsewhere and for barcodes outside the mask."""
    R, B = labels.shape
    w = np.zeros((B, R * n_clusters))
    for r in range(R):
        on = labels[r] >= 0                         # init_labels may leave a barcode out (-1)
        w[np.flatnonzero(on), r * n_clusters + labels[r][on]] = 1.0
    if mask is not None:
        w[~np.asarray(mask, dtype=bool)] = 0.0
    return w


def update_log_pi(col_sum: np.ndarray, restarts: int, n_clusters: int) -> np.ndarray:
    """log pi[R][K] from the E-step's column sums: pi = sum / mass, at least PI_FLOOR, renormalised."""
    cs = np.asarray(col_sum, dtype=np.float64).reshape(restarts, n_clusters)
    mass = cs.sum(axis=1, keepdims=True)
    pi = np.where(mass > 0, cs / np.where(mass > 0, mass, 1.0), 1.0 / n_clusters)
    pi = np.maximum(pi, PI_FLOOR)
    pi /= pi.sum(axis=1, keepdims=True)
    return np.log(pi)


def update_log_pi_active(col_sum: np.ndarray, active: np.ndarray) -> np.ndarray:
    """update_log_pi over the active columns only (active [R][K], at least one per restart): an inactive column keeps log pi = -inf,
    the active ones get pi = sum / mass of the active sums, at least PI_FLOOR, renormalised to sum to 1."""
    act = np.asarray(active, dtype=bool)
    R, K = act.shape
    cs = np.where(act, np.asarray(col_sum, dtype=np.float64).reshape(R, K), 0.0)
    n_act = act.sum(axis=1, keepdims=True)
    mass = cs.sum(axis=1, keepdims=True)
    pi = np.where(mass > 0, cs / np.where(mass > 0, mass, 1.0), 1.0 / n_act)
    pi = np.where(act, np.maximum(pi, PI_FLOOR), 0.0)
    pi /= pi.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        return np.log(pi)


def pair_index(n_clusters: int) -> np.ndarray:
    """[P][2] int: the pairs (k, l), k < l, in the lexicographic order of the doublet components (P = K (K - 1) / 2)."""
    k, l = np.triu_indices(n_clusters, 1)
    return np.stack([k, l], axis=1)


def update_delta(dbl_mass: np.ndarray, n_mask: int) -> np.ndarray:
    """delta[R] from the doublet E-step's per-restart doublet mass and the number of barcodes in the mask, clipped."""
    d = np.asarray(dbl_mass, dtype=np.float64) / max(int(n_mask), 1)
    return np.clip(d, DELTA_MIN, DELTA_MAX)


def converged(prev: Optional[np.ndarray], cur: np.ndarray, tol: float) -> bool:
    """Every restart's |dLL| < tol * |LL|."""
    if prev is None:
        return False
    return bool(np.all(np.abs(cur - prev) < tol * np.abs(cur)))


def best_restart(ll: np.ndarray) -> int:
    """The restart with the highest log-likelihood; on a tie the lowest index."""
    ll = np.asarray(ll, dtype=np.float64)
    return int(np.flatnonzero(ll == ll.max())[0])


def write_em_tsv(path: str, rows: Sequence[Tuple], doublets: bool = False) -> None:
    """<prefix>.em.tsv: one row per (iteration, restart): ITER RESTART LLK PI (the mixing weights the E-step used, comma-joined); with
    doublets, rows (it, r, ll, pi, delta) and a trailing DBL column: the doublet share delta the E-step used."""
    with open(path, "w") as f:
        f.write(EM_HEADER_DBL if doublets else EM_HEADER)
        for row in rows:
            it, r, ll, pi = row[:4]
            f.write(f"{it}\t{r}\t{ll:.6f}\t" + ",".join(f"{x:.6g}" for x in pi) + (f"\t{row[4]:.6g}" if doublets else "") + "\n")


def match_table(llks: np.ndarray, called: np.ndarray, n_clusters: int) -> Tuple[np.ndarray, np.ndarray]:
    """For every cluster k and sample v: the number of barcodes called SNG-CLUSTk (called[b] = k, -1 = not a singlet) and the sum of
    their llks[b][v].  Returns (n_cell[K], sum_llk[K][V])."""
    called = np.asarray(called)
    n = np.bincount(called[called >= 0], minlength=n_clusters)[:n_clusters]
    s = np.zeros((n_clusters, llks.shape[1]))
    for k in range(n_clusters):
        s[k] = llks[called == k].sum(axis=0)
    return n, s


def write_match_tsv(path: str, n_cell: np.ndarray, sum_llk: np.ndarray, sample_ids: Sequence[str], names: Optional[Sequence[str]] = None) -> None:
    """<prefix>.match.tsv: one row per (cluster, genotyped sample); BEST = 1 on the sample with the highest SUM.LLK of a cluster with
    called singlets (the first on a tie).  The clusters are named CLUST0 .. unless `names` are given."""
    names = cluster_ids(sum_llk.shape[0]) if names is None else names
    with open(path, "w") as f:
        f.write(MATCH_HEADER)
        for k in range(sum_llk.shape[0]):
            best = int(np.argmax(sum_llk[k])) if n_cell[k] > 0 else -1
            for v, sm in enumerate(sample_ids):
                f.write(f"{names[k]}\t{sm}\t{int(n_cell[k])}\t{sum_llk[k, v]:.5f}\t{int(v == best)}\n")


def match_labels(truth: np.ndarray, pred: np.ndarray, n_truth: int, n_pred: int) -> np.ndarray:
    """A one-to-one map pred label -> truth label, greedy on the confusion matrix (largest count first; lowest indices on ties).
    Labels < 0 are ignored; a predicted label left without a partner maps to -1."""
    truth, pred = np.asarray(truth), np.asarray(pred)
    ok = (truth >= 0) & (pred >= 0)
    conf = np.zeros((n_pred, n_truth), dtype=np.int64)
    np.add.at(conf, (pred[ok], truth[ok]), 1)
    out = np.full(n_pred, -1, dtype=np.int64)
    used_t = np.zeros(n_truth, dtype=bool)
    for _ in range(min(n_pred, n_truth)):
        c = np.where(out[:, None] >= 0, -1, np.where(used_t[None, :], -1, conf))
        k, t = np.unravel_index(int(np.argmax(c)), c.shape)
        if c[k, t] < 0:
            break
        out[k], used_t[t] = t, True
    return out


# ---- choosing K by a merge path: pure functions the CPU tests reach ---------------------------------------------
def path_score(ev: np.ndarray, n_sing: np.ndarray, n_dbl: int, dbl_score: float, active: np.ndarray) -> Tuple[float, float, float]:
    """The score of one restart's hard-labelled state, (score, evidence, label_term) with score = evidence + dbl_score + label_term:
      evidence    the sum over the active columns k of ev[k], the log marginal likelihood of the reads of the barcodes labelled k;
      dbl_score   the doublet-labelled barcodes' log-likelihoods at the plug-in genotypes;
      label_term  lgamma(Ka) + sum over active k of lgamma(n_k + 1) - lgamma(N_s + Ka): the labels of the N_s singlets among the Ka
                  active clusters, mixing weights integrated out under a flat Dirichlet; + lgamma(n_dbl + 1) + lgamma(N_s + 1)
                  - lgamma(N_s + n_dbl + 2): which barcodes are doublets, their share integrated out under a flat Beta."""
    act = np.asarray(active, dtype=bool)
    n = np.asarray(n_sing, dtype=np.int64)[act]
    ka, ns, nd = int(act.sum()), int(n.sum()), int(n_dbl)
    evidence = float(np.sum(np.asarray(ev, dtype=np.float64)[act]))
    label = lgamma(ka) + sum(lgamma(int(x) + 1) for x in n) - lgamma(ns + ka) + lgamma(nd + 1) + lgamma(ns + 1) - lgamma(ns + nd + 2)
    return evidence + float(dbl_score) + label, evidence, label


def best_active_pair(bf: np.ndarray, active: np.ndarray) -> Tuple[int, int, float]:
    """(k, l, BF) of the pair k < l of two active columns with the largest merge score bf[P] (pair_index order); the lowest pair index
    on a tie.  An emptied column has BF exactly 0 against every column, above the negative scores of distinct donors, so it goes first."""
    act = np.asarray(active, dtype=bool)
    pairs = pair_index(act.shape[0])
    ok = np.flatnonzero(act[pairs[:, 0]] & act[pairs[:, 1]])
    if ok.size == 0:
        raise ValueError("best_active_pair: fewer than two active columns")
    b = np.asarray(bf, dtype=np.float64)[ok]
    p = int(ok[np.flatnonzero(b == b.max())[0]])
    return int(pairs[p][0]), int(pairs[p][1]), float(bf[p])


def path_winner(rows: Sequence[dict]) -> int:
    """The index of the winning row of a merge path: the highest score; on a tie the smaller K, then the lower restart."""
    return max(range(len(rows)), key=lambda i: (rows[i]["score"], -rows[i]["k"], -rows[i]["restart"]))


def write_kpath_tsv(path: str, rows: Sequence[dict]) -> None:
    """<prefix>.kpath.tsv: one row per (step, restart) of the merge path (KPATH_HEADER).  K active clusters; LLK the converged EM's
    log-likelihood there; SCORE = EVIDENCE + DBL.SCORE + LABEL.TERM (path_score); N.SNG / N.DBL the singlet- / doublet-labelled barcodes,
    SIZES the active clusters' singlets in column order; MERGE_K < MERGE_L the pair merged next and BF its merge score (-1, -1 and NA at
    the last step); CHOSEN 1 on the one row whose state the run goes on with."""
    with open(path, "w") as f:
        f.write(KPATH_HEADER)
        for r in rows:
            bf = "NA" if r["merge_k"] < 0 else f"{r['bf']:.6f}"
            f.write(f"{r['step']}\t{r['restart']}\t{r['k']}\t{r['llk']:.6f}\t{r['score']:.6f}\t{r['evidence']:.6f}\t{r['dbl_score']:.6f}\t"
                    f"{r['label_term']:.6f}\t{r['n_sng']}\t{r['n_dbl']}\t" + ",".join(str(int(x)) for x in r["sizes"]) +
                    f"\t{r['merge_k']}\t{r['merge_l']}\t{bf}\t{int(r['chosen'])}\n")


# ---- split-merge moves: pure functions the CPU tests reach ---------------------------------------------------------
def rank_candidates(bf: np.ndarray, gain: np.ndarray, n_merge: int, n_split: int) -> List[Tuple[int, int, int]]:
    """The candidates (k, l, m) of one move: the n_merge pairs (k, l) of highest BF (pair_index order) and the n_split clusters m of highest
    gain, merges outer and splits inner, each in descending score with the lower index first on a tie; a combination with m in {k, l}
    and a split of non-finite gain (a cluster too small to split) are skipped."""
    bf, gain = np.asarray(bf, dtype=np.float64), np.asarray(gain, dtype=np.float64)
    K = gain.shape[0]
    pairs = pair_index(K)
    merges = np.argsort(-bf, kind="stable")[:n_merge]
    ok = np.flatnonzero(np.isfinite(gain))
    splits = ok[np.argsort(-gain[ok], kind="stable")][:n_split]
    return [(int(pairs[p][0]), int(pairs[p][1]), int(m)) for p in merges for m in splits if m not in (pairs[p][0], pairs[p][1])]


def best_candidate(ll: np.ndarray, tol: float) -> int:
    """The candidate to accept: the first (the best ranked) whose converged LL is within tol * |LL| of the highest, since candidates that
    reach the same optimum differ only by the EM's convergence tolerance."""
    ll = np.asarray(ll, dtype=np.float64)
    top = ll.max()
    return int(np.flatnonzero(ll >= top - tol * abs(top))[0])


def split_groups(w: np.ndarray, mask: Optional[np.ndarray] = None) -> np.ndarray:
    """group[B] int32: each barcode's hard label, the argmax of its E-step weights w[B][K] (the lowest cluster on a tie); -1 for a barcode
    outside the mask or with a singlet mass below 0.5 (with em_doublets the weights sum to 1 - the doublet mass)."""
    w = np.asarray(w, dtype=np.float64)
    g = np.argmax(w, axis=1).astype(np.int32) if w.shape[1] else np.zeros(w.shape[0], dtype=np.int32)
    off = w.sum(axis=1) < 0.5
    if mask is not None:
        off |= ~np.asarray(mask, dtype=bool)
    g[off] = -1
    return g


def sub_restart_weights(group: np.ndarray, n_clusters: int, split_restarts: int, seed) -> np.ndarray:
    """w[B][K * Rs * 2]: the one-hot start of the sub-EM.  Sub-restart s of cluster m (restart m * Rs + s, columns 2 (m Rs + s) + {0, 1})
    gives every barcode of group m a random half, drawn from np.random.default_rng(seed) as integers(0, 2, size=(Rs, B)); barcodes of
    group -1 get no weight."""
    group = np.asarray(group, dtype=np.int64)
    B, Rs = group.shape[0], int(split_restarts)
    half = np.random.default_rng(seed).integers(0, 2, size=(Rs, B))
    w = np.zeros((B, n_clusters * Rs * 2))
    idx = np.flatnonzero(group >= 0)
    for s in range(Rs):
        w[idx, 2 * (group[idx] * Rs + s) + half[s, idx]] = 1.0
    return w


def split_gain(ll_sub: np.ndarray, llks: np.ndarray, group: np.ndarray, split_restarts: int) -> Tuple[np.ndarray, np.ndarray]:
    """(gain[K], best[K]): best[m] = the sub-restart of highest LL (the lowest on a tie), gain[m] = max_s ll_sub[m, s] - the sum over the
    barcodes of group m of llks[b][m]; -inf for a cluster of fewer than two barcodes."""
    K = llks.shape[1]
    ll = np.asarray(ll_sub, dtype=np.float64).reshape(K, split_restarts)
    best = np.argmax(ll, axis=1)
    group = np.asarray(group)
    gain = np.full(K, -np.inf)
    for m in range(K):
        mine = group == m
        if np.count_nonzero(mine) >= 2:
            gain[m] = ll[m, best[m]] - llks[mine, m].sum()
    return gain, best


def split_posteriors(w_sub: np.ndarray, group: np.ndarray, best: np.ndarray, split_restarts: int) -> Tuple[np.ndarray, np.ndarray]:
    """(s_a[K][B], s_b[K][B]): the sub-EM posteriors of the two halves of cluster m, from its best sub-restart; a barcode outside group m
    gets 1/2 and 1/2, so that s_a + s_b = 1 and a split keeps all of cluster m's mass."""
    K = len(best)
    group = np.asarray(group)
    s_a, s_b = np.full((K, group.shape[0]), 0.5), np.full((K, group.shape[0]), 0.5)
    for m in range(K):
        mine = group == m
        c = 2 * (m * split_restarts + int(best[m]))
        a, b = w_sub[mine, c], w_sub[mine, c + 1]
        tot = a + b
        s_a[m, mine] = np.where(tot > 0, a / np.where(tot > 0, tot, 1.0), 0.5)
        s_b[m, mine] = 1.0 - s_a[m, mine]
    return s_a, s_b


def candidate_weights(w: np.ndarray, cands: Sequence[Tuple[int, int, int]], s_a: np.ndarray, s_b: np.ndarray) -> np.ndarray:
    """[B][n * K]: candidate j = (k, l, m) is restart j: column k gets w_k + w_l, column l gets w_m * s_a[m], column m gets w_m * s_b[m];
    every other column keeps w."""
    w = np.asarray(w, dtype=np.float64)
    B, K = w.shape
    out = np.empty((B, len(cands) * K))
    for j, (k, l, m) in enumerate(cands):
        c = w.copy()
        c[:, k] = w[:, k] + w[:, l]
        c[:, l] = w[:, m] * s_a[m]
        c[:, m] = w[:, m] * s_b[m]
        out[:, j * K:(j + 1) * K] = c
    return out


def write_moves_tsv(path: str, rows: Sequence[dict]) -> None:
    """<prefix>.moves.tsv: one row per evaluated candidate (MOVES_HEADER); MERGE_K < MERGE_L is the merged pair, SPLIT the split cluster,
    LLK_BEFORE the current LL, LLK_AFTER the candidate's converged LL after ITER iterations, ACCEPTED 1 for the move's accepted candidate."""
    with open(path, "w") as f:
        f.write(MOVES_HEADER)
        for r in rows:
            f.write(f"{r['move']}\t{r['cand']}\t{r['merge_k']}\t{r['merge_l']}\t{r['split']}\t{r['bf']:.6f}\t{r['gain']:.6f}\t"
                    f"{r['ll_before']:.6f}\t{r['ll_after']:.6f}\t{r['iterations']}\t{int(r['accepted'])}\n")


def em_loop(eng, pl, S: int, R: int, K: int, q: np.ndarray, floor: float, log_pi: np.ndarray, delta: np.ndarray, mask, n_mask: int,
            max_iter: int, tol: float, temperature: float, em_doublets: bool, em_rows: Optional[list] = None,
            active: Optional[np.ndarray] = None, it0: int = 0):
    """The EM iterations of R restarts x K clusters after a first M-step (module docstring): returns (ll[R] of the last E-step, log_pi and
    delta after it, iterations).  The engine ends with the M-step of the last E-step's weights.  With `active` ([R][K]; the merge path)
    the inactive columns come with log_pi = -inf and keep it (update_log_pi_active); iterations are numbered from it0 + 1."""
    dense = pl.pair_snp is None
    prev = None
    it = it0
    ll = None
    for it in range(it0 + 1, it0 + max_iter + 1):
        eng.set_genotypes_device(eng.cluster_device_ptr(), S)
        if dense:
            eng.set_pileup(pl)          # a dense pileup's SNP-minor copy of the matrix is made when it is staged
        eng.run_singlet()
        if em_doublets:
            eng.cluster_doublet(R, K)
            ll, cs, dm = eng.cluster_estep_doublet(R, K, log_pi, np.log(delta), temperature, mask)
            if em_rows is not None:
                em_rows += [(it, r, float(ll[r]), np.exp(log_pi[r]), float(delta[r])) for r in range(R)]
            delta = update_delta(dm, n_mask)
        else:
            ll, cs = eng.cluster_estep(R, K, log_pi, temperature, mask)
            if em_rows is not None:
                em_rows += [(it, r, float(ll[r]), np.exp(log_pi[r])) for r in range(R)]
        log_pi = update_log_pi(cs, R, K) if active is None else update_log_pi_active(cs, active)
        eng.cluster_mstep(None, q, floor, fetch=False)
        if converged(prev, ll, tol):
            break
        prev = ll
    return ll, log_pi, delta, it


def merge_path(eng, pl, S: int, R: int, K: int, q: np.ndarray, floor: float, ll: np.ndarray, log_pi: np.ndarray, delta: np.ndarray, mask,
               n_mask: int, max_iter: int, tol: float, temperature: float, em_doublets: bool, k_min: int, em_rows: Optional[list], it: int):
    """The merge path of auto_k (module docstring) from the converged EM at K clusters in `eng`, all R restarts stepping together.  Returns
    (rows of .kpath.tsv with the winner marked; gp[S][K*][3], the winner's hard M-step genotypes of its active columns in ascending
    column order; ll[R], delta[R] and the iteration count at the winner's step)."""
    active = np.ones((R, K), dtype=np.uint8)
    rows: List[dict] = []
    best, g_best, at_best = None, None, None
    # LLD is on the doublet kernel's max-normalised scale, the evidence on K1's sum-normalised one: lsc[b] (a function of the barcode's
    # reads alone) takes a doublet-labelled barcode's LLD to the evidence's scale, as in the doublet E-step
    lsc = eng.cluster_doublet_scale() if em_doublets else None
    for step in range(K - k_min + 1):
        label, n_sing, n_dbl, dsc = eng.cluster_hard(R, K, active, mask, doublets=em_doublets)
        if em_doublets:
            dsc = dsc - np.array([lsc[label[:, r] <= -2].sum() for r in range(R)])
        eng.cluster_mstep(eng.cluster_hard_device_ptr(), q, floor, fetch=False)
        ev, _ = eng.cluster_evidence(R, K, q, floor)
        last = K - step == k_min
        bf = None if last else eng.cluster_merge_score(R, K, q, floor)[0]
        first = len(rows)
        for r in range(R):
            score, evidence, label_term = path_score(ev[r], n_sing[r], n_dbl[r], dsc[r], active[r])
            k, l, b = (-1, -1, float("nan")) if last else best_active_pair(bf[r], active[r])
            rows.append(dict(step=step, restart=r, k=K - step, llk=float(ll[r]), score=score, evidence=evidence, dbl_score=float(dsc[r]),
                             label_term=label_term, n_sng=int(n_sing[r][active[r] > 0].sum()), n_dbl=int(n_dbl[r]),
                             sizes=n_sing[r][active[r] > 0].tolist(), merge_k=k, merge_l=l, bf=b, chosen=False))
        w = path_winner(rows)
        if w >= first:                      # a state of this step is the best so far: keep its genotypes
            best = w
            gp = eng.cluster_genotypes(S)
            cols = rows[w]["restart"] * K + np.flatnonzero(active[rows[w]["restart"]])
            g_best = np.ascontiguousarray(gp[:, cols, :])
            at_best = (ll, delta, it)
        if last:
            break
        frm = np.array([rows[first + r]["merge_l"] for r in range(R)], dtype=np.int32)
        into = np.array([rows[first + r]["merge_k"] for r in range(R)], dtype=np.int32)
        eng.cluster_merge_columns(R, K, frm, into)
        log_pi = np.array(log_pi, dtype=np.float64)
        for r in range(R):
            log_pi[r, into[r]] = np.logaddexp(log_pi[r, into[r]], log_pi[r, frm[r]])
            log_pi[r, frm[r]] = -np.inf
            active[r, frm[r]] = 0
        eng.cluster_mstep(None, q, floor, fetch=False)
        ll, log_pi, delta, it = em_loop(eng, pl, S, R, K, q, floor, log_pi, delta, mask, n_mask, max_iter, tol, temperature, em_doublets,
                                        em_rows, active=active, it0=it)
    rows[best]["chosen"] = True
    return rows, g_best, at_best[0], at_best[1], at_best[2]


def sub_em(eng, pl, S: int, K: int, Rs: int, q: np.ndarray, floor: float, w0: np.ndarray, group: np.ndarray, max_iter: int, tol: float):
    """The 2-component sub-EM inside every cluster at once: restarts m * Rs + s of K * Rs, the grouped E-step restricting restart r to
    group r // Rs.  Returns (ll[K * Rs], the last E-step's weights [B][K * Rs * 2])."""
    R2 = K * Rs
    dense = pl.pair_snp is None
    eng.cluster_mstep(w0, q, floor, fetch=False)
    log_pi = np.full((R2, 2), -np.log(2.0))
    prev = None
    for _ in range(max_iter):
        eng.set_genotypes_device(eng.cluster_device_ptr(), S)
        if dense:
            eng.set_pileup(pl)
        eng.run_singlet()
        ll, cs = eng.cluster_estep_grouped(R2, 2, log_pi, group, Rs)
        log_pi = update_log_pi(cs, R2, 2)
        eng.cluster_mstep(None, q, floor, fetch=False)
        if prev is not None and np.all(np.abs(ll - prev) <= tol * np.abs(ll)):    # <=: an empty group's LL stays exactly 0
            break
        prev = ll
    return ll, eng.cluster_weights()


def _staged_engine(V: int, pl, S: int, alphas, doublet_prior: float, device: int, mode: int):
    e = engine.Engine(V, alphas, doublet_prior, device=device, mode=mode)
    e.set_genotypes(np.full((S, V, 3), 1.0 / 3.0, dtype=np.float32))
    e.set_pileup(pl)
    e.cluster_stage()
    return e


def split_merge_moves(eng, r_cur: int, R_cur: int, ll_cur: float, delta_cur: float, pl, S: int, K: int, q: np.ndarray, floor: float, mask,
                      n_mask: int, max_iter: int, tol: float, temperature: float, em_doublets: bool, seed: int, max_moves: int,
                      candidates: Sequence[int], split_restarts: int, alphas, doublet_prior: float, device: int, mode: int):
    """Split-merge moves from restart r_cur of R_cur restarts in `eng` (whose last M-step holds that restart's final weights): merge
    scores, the sub-EM, the candidates as restarts of a normal EM, acceptance by converged LL; repeated until a move is rejected or
    max_moves.  Returns (gp[S][K][3] of the accepted state, or None when no move was accepted; the rows of .moves.tsv).  The engines it
    makes are closed; `eng` is left to the caller."""
    rows: List[dict] = []
    if K < 3 or max_moves < 1:
        return None, rows                  # K = 2: every split overlaps the merged pair
    Rs = int(split_restarts)
    n_merge, n_split = (int(x) for x in candidates)
    cur, cur_owned, g_acc = eng, False, None
    sub = _staged_engine(K * Rs * 2, pl, S, alphas, doublet_prior, device, mode)
    try:
        for move in range(1, max_moves + 1):
            bf, _ = cur.cluster_merge_score(R_cur, K, q, floor)
            bf = bf[r_cur]
            w_cur = cur.cluster_weights()[:, r_cur * K:(r_cur + 1) * K]
            llks = cur.get_singlet()[0][:, r_cur * K:(r_cur + 1) * K]
            group = split_groups(w_cur, mask)
            ll_sub, w_sub = sub_em(sub, pl, S, K, Rs, q, floor, sub_restart_weights(group, K, Rs, [seed, move]), group, max_iter, tol)
            gain, best = split_gain(ll_sub, llks, group, Rs)
            cands = rank_candidates(bf, gain, n_merge, n_split)
            if not cands:
                break
            s_a, s_b = split_posteriors(w_sub, group, best, Rs)
            wc = candidate_weights(w_cur, cands, s_a, s_b)
            n = len(cands)
            ce = _staged_engine(n * K, pl, S, alphas, doublet_prior, device, mode)
            try:
                ce.cluster_mstep(wc, q, floor, fetch=False)
                log_pi = update_log_pi(wc.sum(axis=0), n, K)
                ll_c, _, delta_c, it_c = em_loop(ce, pl, S, n, K, q, floor, log_pi, np.full(n, delta_cur), mask, n_mask, max_iter, tol,
                                                 temperature, em_doublets)
            except BaseException:
                ce.close()
                raise
            j = best_candidate(ll_c, tol)
            ok = bool(ll_c[j] - ll_cur > tol * abs(ll_cur))
            pairs = {(k, l): p for p, (k, l) in enumerate(pair_index(K).tolist())}
            for c, (k, l, m) in enumerate(cands):
                rows.append(dict(move=move, cand=c, merge_k=k, merge_l=l, split=m, bf=float(bf[pairs[(k, l)]]), gain=float(gain[m]),
                                 ll_before=float(ll_cur), ll_after=float(ll_c[c]), iterations=it_c, accepted=ok and c == j))
            if not ok:
                ce.close()
                break
            if cur_owned:
                cur.close()
            cur, cur_owned, r_cur, R_cur = ce, True, j, n
            ll_cur, delta_cur = float(ll_c[j]), float(delta_c[j])
            _, _, gp = cur.get_cluster(S)
            g_acc = np.ascontiguousarray(gp[:, j * K:(j + 1) * K, :])
    finally:
        sub.close()
        if cur_owned:
            cur.close()
    return g_acc, rows


def cluster_run(store_or_pileup, n_clusters: int, out_prefix: str, restarts: int = 16, seed: int = 0, max_iter: int = 50, tol: float = 1e-7,
                floor: float = 1e-3, min_snp: int = 0, alphas: Sequence[float] = (0.0, 0.5), rounds: int = 1,
                match: Optional[Tuple[np.ndarray, Sequence[str]]] = None, barcodes: Optional[Sequence[str]] = None, device: int = 0,
                mode: int = capi.DMX_MODE_STRICT, doublet_prior: float = 0.5, temperature: float = 1.0,
                snps: Optional[Sequence[Tuple]] = None, em_doublets: bool = False, init_labels: Optional[np.ndarray] = None,
                split_merge: bool = False, sm_max_moves: Optional[int] = None, sm_candidates: Sequence[int] = SM_CANDIDATES,
                sm_split_restarts: int = SM_SPLIT_RESTARTS, auto_k: bool = False, k_min: int = 2) -> dict:
    """EM clustering of the barcodes of `store_or_pileup` (a Store, or a HostPileup with barcodes=...) into n_clusters donors, then
    the final demultiplexing pass and `rounds` hard-refine rounds (module docstring).  `match` = (g[S][NV][3], sample_ids) scores each
    cluster against genotyped samples (<prefix>.match.tsv).  `init_labels` ([R][B] int, values in [-1, K); -1 = no weight in the first
    M-step) replaces the seeded random start, e.g. to start from an earlier clustering; its R replaces `restarts`.  With split_merge the
    winning restart goes through split-merge moves (at most sm_max_moves, default K; sm_candidates = (merges, splits) per move,
    sm_split_restarts random-half sub-restarts per split) and <prefix>.moves.tsv records every candidate.  With auto_k n_clusters is
    K_max: the restarts walk a merge path down to k_min clusters and the state of highest score gives K (module docstring;
    <prefix>.kpath.tsv); not together with split_merge.  Returns a dict: the winning restart, per-restart LL, iterations, the cluster
    genotype matrix gp[S][K][3] and the prior q[S][3]; with em_doublets also `delta`, the winning restart's doublet share; with
    split_merge also `moves`, the rows of .moves.tsv; with auto_k also `n_clusters`, the chosen K, and `kpath`, the rows of .kpath.tsv."""
    if isinstance(store_or_pileup, engine.HostPileup):
        pl = store_or_pileup
        if barcodes is None:
            raise ValueError("cluster_run: a HostPileup needs barcodes=")
    else:
        pl, barcodes = store_or_pileup.freeze(), store_or_pileup.barcodes()
    B, S, K, R = pl.n_cells, pl.n_snps, int(n_clusters), int(restarts)
    if init_labels is not None:
        init_labels = check_init_labels(init_labels, B, K)
        R = init_labels.shape[0]
    check_args(K, R, max_iter, tol, floor, B, len(pl.pair_nrd))
    if auto_k:
        check_auto_k_args(K, int(k_min), split_merge)
    if split_merge:
        check_sm_args(K, sm_candidates, sm_split_restarts, sm_max_moves)
    C = R * K
    mask = pl.n_snp_per_cell >= min_snp if min_snp > 0 else None
    kw = dict(barcodes=barcodes, doublet_prior=doublet_prior, device=device, mode=mode, min_snp=min_snp)
    eng = engine.Engine(C, alphas, doublet_prior, device=device, mode=mode)
    moves: List[dict] = []
    kpath: List[dict] = []
    em_rows = []
    try:
        # prior: pooled REF / ALT counts of every barcode (one refinement with all barcodes in column 0)
        flat = np.full((S, C, 3), 1.0 / 3.0, dtype=np.float32)
        eng.set_genotypes(flat)
        eng.set_pileup(pl)
        _, _, n_ref, n_alt, _ = eng.refine_genotypes(np.zeros(B, dtype=np.int32), flat, floor)
        del flat
        q = hwe_prior(n_ref[:, 0], n_alt[:, 0])
        eng.cluster_stage()
        # first M-step from each restart's random hard assignment, pi uniform
        labels = init_labels if init_labels is not None else initial_labels(seed, R, B, K)
        eng.cluster_mstep(one_hot_weights(labels, K, mask), q, floor, fetch=False)
        log_pi = np.full((R, K), -np.log(K))
        delta = np.full(R, DELTA0)
        n_mask = B if mask is None else int(np.count_nonzero(mask))
        ll, log_pi, delta, it = em_loop(eng, pl, S, R, K, q, floor, log_pi, delta, mask, n_mask, max_iter, tol, temperature, em_doublets,
                                        em_rows)
        if auto_k:
            kpath, g, ll, delta, it = merge_path(eng, pl, S, R, K, q, floor, ll, log_pi, delta, mask, n_mask, max_iter, tol, temperature,
                                                 em_doublets, int(k_min), em_rows, it)
            win = next(row["restart"] for row in kpath if row["chosen"])
            K = g.shape[1]                  # K*: everything below runs at the chosen K
        else:
            win = best_restart(ll)
            _, _, gp = eng.get_cluster(S)
            g = np.ascontiguousarray(gp[:, win * K:(win + 1) * K, :])
        if split_merge:
            g_sm, moves = split_merge_moves(eng, win, R, float(ll[win]), float(delta[win]), pl, S, K, q, floor, mask, n_mask, max_iter, tol,
                                            temperature, em_doublets, seed, K if sm_max_moves is None else int(sm_max_moves), sm_candidates,
                                            sm_split_restarts, alphas, doublet_prior, device, mode)
            if g_sm is not None:
                g = g_sm
    finally:
        eng.close()
    write_em_tsv(out_prefix + ".em.tsv", em_rows, doublets=em_doublets)
    if split_merge:
        write_moves_tsv(out_prefix + ".moves.tsv", moves)
    if auto_k:
        write_kpath_tsv(out_prefix + ".kpath.tsv", kpath)
    ids = cluster_ids(K)
    engine.demuxlet_run(pl, g, ids, alphas, out_prefix, **kw)
    # hard-refine rounds: the previous round's singlets only, prior q for every cluster
    qk = np.ascontiguousarray(np.broadcast_to(q[:, None, :], (S, K, 3)))
    reng = engine.Engine(K, alphas, doublet_prior, device=device, mode=mode)
    try:
        reng.set_genotypes(qk)
        reng.set_pileup(pl)
        prev_prefix = out_prefix
        for r in range(1, max(rounds, 1) + 1):
            assign = refine.assignments_from_best(prev_prefix + ".best", ids, barcodes)
            ll_r, n_cell, n_ref_r, n_alt_r, gr = reng.refine_genotypes(assign, qk, floor)
            if r > rounds:
                break                       # rounds = 0: the refinement only feeds <prefix>.clust.tsv
            prev_prefix = f"{out_prefix}.r{r}"
            engine.demuxlet_run(pl, gr, ids, alphas, prev_prefix, **kw)
    finally:
        reng.close()
    refine.write_refined_tsv(out_prefix + ".clust.tsv", snps, ids, ll_r, n_cell, n_ref_r, n_alt_r, gr)
    if match is not None:
        mg, msamples = match
        mg = np.ascontiguousarray(mg, dtype=np.float32)
        if mg.shape[0] != S or mg.shape[1] != len(msamples):
            raise ValueError(f"match: genotype matrix {mg.shape} for {S} SNPs and {len(msamples)} samples")
        meng = engine.Engine(len(msamples), alphas, doublet_prior, device=device, mode=mode)
        try:
            meng.set_genotypes(mg)
            meng.set_pileup(pl)
            meng.run_singlet()
            llks, _ = meng.get_singlet()
        finally:
            meng.close()
        called = refine.assignments_from_best(prev_prefix + ".best", ids, barcodes)
        n_cell_m, sum_llk = match_table(llks, called, K)
        write_match_tsv(out_prefix + ".match.tsv", n_cell_m, sum_llk, msamples)
    res = dict(restart=win, ll=ll, iterations=it, gp=g, prior=q, last_prefix=prev_prefix)
    if em_doublets:
        res["delta"] = float(delta[win])
    if split_merge:
        res["moves"] = moves
    if auto_k:
        res["n_clusters"], res["kpath"] = K, kpath
    return res


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.cluster", description="genotype-free demultiplexing: EM clustering into K donors")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--n-clusters", type=int, required=True, help="K, the number of donors in the pool")
    ap.add_argument("--out", required=True, help="output prefix: <out>.best/.single/.sing2, <out>.r<N>.*, <out>.em.tsv, <out>.clust.tsv")
    ap.add_argument("--restarts", type=int, default=16, help="independent random starts; the best log-likelihood wins (default 16)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--tol", type=float, default=1e-7, help="stop when every restart's |dLL| < tol * |LL| (default 1e-7)")
    ap.add_argument("--floor", type=float, default=1e-3, help="added to the prior of every covered row (default 1e-3)")
    ap.add_argument("--min-snp", type=int, default=0, help="barcodes with fewer covered SNPs take no part in the EM and get no call")
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.0, 0.5], help="grid of alpha values (default 0 0.5)")
    ap.add_argument("--doublet-prior", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=1, help="hard-refine rounds after the final pass (default 1)")
    ap.add_argument("--match", action="store_true", help="score the clusters against the dump's genotyped samples (<out>.match.tsv)")
    ap.add_argument("--em-doublets", action="store_true",
                    help="doublet components (alpha = 0.5) for every pair of clusters in the EM; <out>.em.tsv gains a DBL column")
    ap.add_argument("--split-merge", action="store_true",
                    help="split-merge moves on the winning restart after the EM (DESIGN.md section 16); writes <out>.moves.tsv")
    ap.add_argument("--sm-max-moves", type=int, default=None, help="at most this many accepted moves (default K)")
    ap.add_argument("--sm-candidates", type=int, nargs=2, default=list(SM_CANDIDATES), metavar=("MERGES", "SPLITS"),
                    help="top merges x top splits evaluated per move (default 3 3)")
    ap.add_argument("--sm-split-restarts", type=int, default=SM_SPLIT_RESTARTS, help="random-half sub-restarts per split (default 4)")
    ap.add_argument("--auto-k", action="store_true",
                    help="choose the number of donors: --n-clusters is an upper bound K_max (about twice the expected number), a merge "
                         "path down to --k-min is scored by model evidence (DESIGN.md section 20); writes <out>.kpath.tsv")
    ap.add_argument("--k-min", type=int, default=None, help="with --auto-k: the smallest number of clusters the path reaches (default 2)")
    ap.add_argument("--fast", action="store_true", help="DMX_MODE_FAST for every pass")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    if a.n_clusters < 2:
        ap.error("--n-clusters must be at least 2")
    if a.restarts < 1 or a.n_clusters * a.restarts > MAX_COLUMNS:
        ap.error(f"--restarts x --n-clusters must be in [1, {MAX_COLUMNS}]")
    if a.k_min is not None and not a.auto_k:
        ap.error("--k-min needs --auto-k")
    if a.auto_k:
        a.k_min = 2 if a.k_min is None else a.k_min
        try:
            check_auto_k_args(a.n_clusters, a.k_min, a.split_merge)
        except ValueError as e:
            ap.error(str(e))
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    d = refine.read_pileup_txt(a.pileup)
    match = None
    if a.match:
        if not d.sample_ids:
            raise SystemExit(f"--match: {a.pileup} has no genotyped samples")
        match = (d.g, d.sample_ids)
    cluster_run(d.pileup, a.n_clusters, a.out, restarts=a.restarts, seed=a.seed, max_iter=a.max_iter, tol=a.tol, floor=a.floor,
                min_snp=a.min_snp, alphas=a.alpha, rounds=a.rounds, match=match, barcodes=d.barcodes, device=a.gpu,
                mode=capi.DMX_MODE_FAST if a.fast else capi.DMX_MODE_STRICT, doublet_prior=a.doublet_prior, snps=d.snps,
                em_doublets=a.em_doublets, split_merge=a.split_merge, sm_max_moves=a.sm_max_moves, sm_candidates=tuple(a.sm_candidates),
                sm_split_restarts=a.sm_split_restarts, auto_k=a.auto_k, k_min=2 if a.k_min is None else a.k_min)
    return 0


if __name__ == "__main__":
    sys.exit(main())
