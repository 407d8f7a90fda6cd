"""Test-side pileups for the quality-range tests: base-quality profiles (demuxlet_amd.synth.draw_bq), a depth mix that reaches every
read-count regime of the kernels, and adversarial allele patterns; plus the glue that feeds such a pileup to the engine and the oracle.

Depth mix of a covered pair: 0..6 reads (the seed tables' whole answers and the first reads of the loop), 14..17 (both sides of
kSafeReads = 15, the reciprocal-refined division), 40, and optionally a few pairs of 256..300 reads (u16 read counts).
Adversarial pairs: every read ALT on a row where the pair's source sample is hom-REF, every read REF where it is hom-ALT — the
likelihoods that shrink fastest per read (one read at quality 127 scales them by about err(127)/3)."""
import numpy as np

from demuxlet_amd import synth

DEPTHS = np.array([0, 1, 2, 3, 4, 5, 6, 14, 15, 16, 17, 40])
DEPTH_P = np.array([0.04, 0.34, 0.2, 0.1, 0.06, 0.04, 0.04, 0.04, 0.04, 0.04, 0.04, 0.02])


def mixed_depth_pileup(rng, alleles, B, delta, quals="edges", dense=False, deep=0, adversarial=0.15, doublet_rate=0.2,
                       depths=None):
    """A synth.SynthPileup over alleles [S][V][2]: cell c is sample c mod V (a doublet with another sample w.p. doublet_rate), each
    SNP covered w.p. delta (every SNP when dense), pair depths from DEPTHS (or the given `depths`, drawn uniformly), `deep` pairs of
    256..300 reads (u16 counts), a fraction `adversarial` of the pairs all-ALT on a hom-REF source row / all-REF on a hom-ALT one,
    qualities from the profile `quals`.  Every read is kept (allele 0 or 1)."""
    S, V, _ = alleles.shape
    dosage = np.clip(alleles, 0, 1).sum(axis=2)
    s1 = np.arange(B) % V
    s2 = np.where((rng.random(B) < doublet_rate) & (V > 1), (s1 + 1 + rng.integers(0, max(V - 1, 1), size=B)) % V, -1)
    cov = np.ones((B, S), dtype=bool) if dense else rng.random((B, S)) < delta
    cc, ss = np.nonzero(cov)
    P = len(cc)
    if depths is None:
        nrd = rng.choice(DEPTHS, size=P, p=DEPTH_P)
    else:
        nrd = rng.choice(np.asarray(depths), size=P)
    if deep and P:
        nrd[rng.choice(P, size=min(deep, P), replace=False)] = rng.integers(256, 301, size=min(deep, P))
    pr = np.repeat(np.arange(P), nrd)
    src = np.where((s2[cc[pr]] >= 0) & (rng.random(len(pr)) < 0.5), s2[cc[pr]], s1[cc[pr]])
    alt = rng.random(len(pr)) < dosage[ss[pr], src] / 2.0
    adv = rng.random(P) < adversarial
    d1 = dosage[ss, s1[cc]]
    alt = np.where(adv[pr] & (d1[pr] == 0), True, alt)
    alt = np.where(adv[pr] & (d1[pr] == 2), False, alt)
    bq = synth.draw_bq(rng, len(pr), quals)
    reads = (bq | (alt.astype(np.uint8) << 7)).astype(np.uint8)
    cpo = np.concatenate([[0], np.cumsum(cov.sum(axis=1))]).astype(np.int64)
    cro = np.concatenate([[0], np.cumsum(np.bincount(cc, weights=nrd, minlength=B))]).astype(np.int64)
    totl = np.bincount(cc, weights=nrd, minlength=B).astype(np.int32)
    truth = np.stack([s1, s2], axis=1).astype(np.int32)
    nrd = nrd.astype(np.uint8 if P == 0 or nrd.max() <= 255 else np.uint16)
    return synth.SynthPileup(B, S, cpo, cro, None if dense else ss.astype(np.int32), nrd, reads, totl, totl.copy(), totl.copy(), truth)


def genotypes(eng, rng, alleles, field, gt_error=0.01):
    """float32 [S][V][3] genotype matrix of a field (the engine's own converters)."""
    S = alleles.shape[0]
    if field == "GT":
        return np.stack([eng.geno_from_gt(alleles[s], gt_error) for s in range(S)])
    if field == "GP":
        return np.stack([eng.geno_from_gp(x, gt_error) for x in synth.raw_gp_from_alleles(rng, alleles)])
    if field == "PL":
        return np.stack([eng.geno_from_pl(x) for x in synth.raw_pl_from_alleles(rng, alleles)])
    raise ValueError(field)


def host_pileup(eng, sp):
    return eng.HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads,
                          sp.rd_totl, sp.rd_pass, sp.rd_uniq)


def oracle_csr(oracle, sp, barcodes=None):
    """The oracle's CSR of a C-ABI pileup (words rebuilt from the packed read bytes)."""
    words = ((sp.reads >> 7).astype(np.uint32) << 24) | ((sp.reads & 0x7F).astype(np.uint32) << 16) | 1
    pair_snp = sp.pair_snp if sp.pair_snp is not None else np.tile(np.arange(sp.n_snps, dtype=np.int32), sp.n_cells)
    return oracle.Csr(list(barcodes) if barcodes is not None else [f"c{i:06d}" for i in range(sp.n_cells)], sp.cell_pair_off, pair_snp,
                      np.concatenate([[0], np.cumsum(sp.pair_nrd.astype(np.int64))]), words.astype(np.uint32), sp.rd_totl, sp.rd_pass,
                      sp.rd_uniq)


def oracle_run(oracle, sp, g, alphas=(0.0, 0.5), prior=0.5, singlet_only=False):
    return oracle.run_csr(oracle_csr(oracle, sp), [f"s{j}" for j in range(g.shape[1])], g, oracle.Params(tuple(alphas), prior), None,
                          singlet_only)
