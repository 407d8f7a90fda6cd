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


A2, A3 = (0.0, 0.5), (0.0, 0.25, 0.5)
# (case id, field, V, alphas, mode, switches, K1 name prefix, K2 name prefix, dense, u16 pairs).  Which V / field / switch picks a family:
# launch_singlet and launch_doublet in dmx_engine.hip.  k_singlet_can(p) need one-byte read counts, so their cases have no u16 pairs.
FAMILIES = [
    # K1
    ("k1_singlet", "GP", 8, A2, "strict", {}, "k_singlet<", "k_doublet_a2<", False, 3),
    ("k1_singlet_own", "GP", 16, A2, "strict", {}, "k_singlet_own<", "k_doublet_a2u16", False, 3),
    ("k1_singlet_cls", "GT", 18, A2, "strict", {}, "k_singlet_cls<", "k_doublet_cls<", False, 3),
    ("k1_singlet_can", "GT", 8, A2, "strict", {}, "k_singlet_can<", "k_doublet_cls<", False, 0),
    ("k1_singlet_canp", "GT", 8, A2, "strict", {"DMX_K1_CANP": "1"}, "k_singlet_canp<", "k_doublet_cls<", True, 0),
    ("k1_singlet_clsw", "GT", 40, A2, "strict", {}, "k_singlet_clsw<", "k_doublet_clsp<", False, 3),
    ("k1_wide_v129_gp", "GP", 129, A2, "strict", {}, "k_singlet<", "k_doublet_a2<", False, 2),
    ("k1_wide_v129_gt", "GT", 129, A2, "strict", {}, "k_singlet_clsw<", "k_doublet_cls<", False, 2),
    # K2
    ("k2_cls_v24", "GT", 24, A2, "strict", {}, "k_singlet_clsw<", "k_doublet_cls<", False, 3),
    ("k2_clsp_fast", "GT", 40, A2, "fast", {}, "k_singlet_clsw<", "k_doublet_clsp<", False, 3),
    ("k2_clsym", "GT", 8, A2, "fast", {}, "k_singlet_cls<", "k_doublet_clsym<", False, 3),
    ("k2_clsym_v24", "GT", 24, A2, "fast", {}, "k_singlet_clsw<", "k_doublet_clsym<", False, 3),
    ("k2_clsn", "GT", 16, A3, "strict", {}, "k_singlet_cls<", "k_doublet_clsn<", False, 3),
    ("k2_a2u16", "GP", 16, A2, "strict", {}, "k_singlet_own<", "k_doublet_a2u16", False, 3),
    ("k2_a2u", "GP", 32, A2, "strict", {}, "k_singlet_own<", "k_doublet_a2u<", False, 3),
    ("k2_a2", "GP", 32, A2, "strict", {"DMX_A2_NO_SYMU": "1"}, "k_singlet_own<", "k_doublet_a2<", True, 0),
    ("k2_a2s", "GP", 32, A2, "strict", {"DMX_A2_SYM": "1"}, "k_singlet_own<", "k_doublet_a2s<", False, 3),
    ("k2_sym_v8", "GP", 8, A2, "fast", {}, "k_singlet<", "k_doublet_sym<", False, 3),
    ("k2_sym_v32", "PL", 32, A2, "fast", {}, "k_singlet_own<", "k_doublet_sym<", True, 0),
    ("k2_an", "PL", 16, A3, "strict", {}, "k_singlet_own<", "k_doublet_an<", False, 3),
    ("k2_anf", "GP", 16, A3, "fast", {}, "k_singlet_own<", "k_doublet_anf<", False, 3),
    ("k2_a2f", "GP", 16, (0.0, 0.25), "fast", {"DMX_NO_ANF": "1"}, "k_singlet_own<", "k_doublet_a2f<", False, 3),
    ("k2_generic", "GP", 8, A2, "strict", {"DMX_K2_GENERIC": "1"}, "k_singlet<", "k_doublet_generic<", False, 3),
    # K2 on DENSE pileups of 32 / 16 soft-field samples (family_problem: S = 131 = four tiles and three pairs, B = 11 = five two-barcode workgroups
    # and a lone last barcode): the two-barcode kernel (the headline) and its forms, the one-barcode kernel on the same layout, k_doublet_a2u16.
    # The K2 names are whole names (kernel_named below tells k_doublet_a2u16 from its fall-back form, which the prefix alone does not).
    ("k2_a2u2", "GP", 32, A2, "strict", {}, "k_singlet_own<", "k_doublet_a2u<k_doublet_a2u2>", True, 3),
    ("k2_a2u2_diag_behind", "GP", 32, A2, "strict", {"DMX_A2U2_NO_DIAG": "1"}, "k_singlet_own<", "k_doublet_a2u<k_doublet_a2u2_whole_diag_behind>", True, 3),
    ("k2_a2u2_mirror_fallback", "GP", 32, A2, "strict", {"DMX_A2U_MIRROR_FALLBACK": "1"}, "k_singlet_own<", "k_doublet_a2u<k_doublet_a2u2_mirror_fallback>",
     True, 3),
    ("k2_a2u_dense_one_barcode", "GP", 32, A2, "strict", {"DMX_A2U_ONE_BARCODE": "1"}, "k_singlet_own<", "k_doublet_a2u<4>", True, 3),
    ("k2_a2u16_dense", "GP", 16, A2, "strict", {}, "k_singlet_own<", "k_doublet_a2u16", True, 3),
    ("k2_a2u16_mirror_fallback", "GP", 16, A2, "strict", {"DMX_A2U_MIRROR_FALLBACK": "1"}, "k_singlet_own<", "k_doublet_a2u16_mirror_fallback", True, 3),
]


def kernel_named(name, want):
    """kernel_names reported `want`: as a prefix when `want` ends inside a template argument list ("k_doublet_a2<"), as the whole name
    otherwise (the name itself, or the name and a parameter list) — "k_doublet_a2u16" is not "k_doublet_a2u16_mirror_fallback"."""
    return name.startswith(want) and (want.endswith("<") or name == want or name.startswith(want + "("))


def family_problem(eng, case, field, V, dense, deep, quals):
    seed = 31000 + 7 * V + sum(map(ord, case)) + {"full": 0, "edges": 1, "max": 2}[quals]
    rng = np.random.default_rng(seed)
    S, B = (131, 11) if dense else ((220, 12) if V > 64 else (300, 24))
    raw = synth.make_raw_genotypes(rng, S, V)
    g = genotypes(eng, rng, raw.alleles, field)
    sp = mixed_depth_pileup(rng, raw.alleles, B, 0.3, quals=quals, dense=dense, deep=deep)
    return g, sp


SWITCHES = ("DMX_K1_CANP", "DMX_A2_NO_SYMU", "DMX_A2_SYM", "DMX_NO_ANF", "DMX_K2_GENERIC", "DMX_FINALS_ANY_DEPTH", "DMX_SYM_NO_FINALS",
            "DMX_A2_NO_FINALS", "DMX_SYM_NO_SEEDS", "DMX_A2_NO_SEEDS", "DMX_CERTIFY_NO_FINALS", "DMX_CERTIFY_NO_SEEDS", "DMX_NO_CLASSES",
            "DMX_K1_NO_CANP", "DMX_K1_NO_LEAN", "DMX_K1_NO_OWN", "DMX_A2U_ONE_BARCODE", "DMX_A2U2_NO_DIAG", "DMX_A2U_MIRROR_FALLBACK",
            "DMX_A2U_DIAG_WAVE")
TABLES = {
    "tables_default": {},
    "tables_off": {k: "1" for k in ("DMX_SYM_NO_FINALS", "DMX_A2_NO_FINALS", "DMX_SYM_NO_SEEDS", "DMX_A2_NO_SEEDS", "DMX_CERTIFY_NO_FINALS",
                                    "DMX_CERTIFY_NO_SEEDS")},
    "tables_any_depth": {"DMX_FINALS_ANY_DEPTH": "1"},
}


def run_with_env(eng, monkeypatch, g, sp, alphas, mode, env, stage=None, split=False):
    """One engine run under the switches `env`.  stage(engine): the caller's own way of handing the pileup over (default: set_pileup of the host
    arrays); what it returns is kept alive until the engine is closed.  split: run_singlet + run_doublet in place of dmx_engine_run."""
    from demuxlet_amd import capi
    monkeypatch.setenv("DMX_EXPERIMENTS", "1")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = eng.Engine(g.shape[1], alphas, 0.5, mode=capi.DMX_MODE_FAST if mode == "fast" else capi.DMX_MODE_STRICT)
    e.set_genotypes(g)
    keep = stage(e) if stage else e.set_pileup(host_pileup(eng, sp))
    if split:
        e.run_singlet(); e.run_doublet()
    else:
        e.run()
    e.sync()
    names = e.kernel_names()
    llks, llk0s = e.get_singlet()
    grid, l00, summ = e.get_doublet()
    e.close()
    return dict(llks=llks, llk0s=llk0s, grid=grid, l00=l00, summ=summ, names=names)
