"""The small unevenly loaded pool that the prior tests share (CPU recovery test, GPU end-to-end test): 6 donors of the VCF with shares
0.4 .. 0.05 and one absent, 600 barcodes of about 60 SNPs, a fifth of the droplets holding two cells."""
import numpy as np

SEED = 2025
V, S, B = 6, 300, 600
DELTA, RBAR = 0.2, 1.5
SHARES = (0.40, 0.25, 0.20, 0.10, 0.05, 0.0)
DOUBLET_RATE = 0.2
ALPHAS = (0.0, 0.5)
ABSENT = 5
CAP_ABSENT, CAP_SHARE, CAP_RATE = 1e-3, 0.05, 0.05      # the recovery conditions


def make(synth, geno_from_gt):
    """(pileup, truth, g[S][V][3] float32) from demuxlet_amd.synth and a geno_from_gt (the engine's or the oracle's: same rows)."""
    rng = np.random.default_rng(SEED)
    raw = synth.make_raw_genotypes(rng, S, V)
    sp, truth = synth.make_pool_pileup(rng, raw.alleles, B, DELTA, RBAR, SHARES, DOUBLET_RATE)
    g = np.asarray(geno_from_gt(raw.alleles, 0.01), dtype=np.float32).reshape(S, V, 3)
    return sp, truth, g


def oracle_grid(O, sp, g):
    """The CPU oracle's llksAB[B][V][V][A] on ALPHAS."""
    po = np.asarray(sp.cell_pair_off, dtype=np.int64)
    snp = sp.pair_snp if sp.pair_snp is not None else (np.arange(po[-1]) - np.repeat(po[:-1], np.diff(po))).astype(np.int32)
    reads = np.asarray(sp.reads)
    words = ((reads >> 7).astype(np.uint32) << 24) | ((reads & 0x7F).astype(np.uint32) << 16) | 1
    csr = O.Csr([f"c{i}" for i in range(sp.n_cells)], sp.cell_pair_off, snp, np.concatenate([[0], np.cumsum(sp.pair_nrd.astype(np.int64))]),
                words.astype(np.uint32), sp.rd_totl, sp.rd_pass, sp.rd_uniq)
    return O.run_csr(csr, [f"s{j}" for j in range(g.shape[1])], g, O.Params(ALPHAS, 0.5)).llksAB.reshape(sp.n_cells, V, V, len(ALPHAS))
