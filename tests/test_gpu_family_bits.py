"""GPU (-m gpu): the bits every K1 / K2 kernel family, k_doublet_diag, k_certify and K3 produce, pinned.

For every case of quality_mix.FAMILIES, every base-quality profile and every entry of quality_mix.TABLES the engine runs family_problem
and a SHA-256 over the bytes of llks, llk0s, grid, l00 and the named fields of the K3 records (field by field, so the struct's padding
cannot enter) is compared with tests/golden/family_bits.json.  The file also holds a hash of each problem's inputs (the genotype matrix
and the pileup arrays), checked first: a drift of synth or quality_mix then fails as "inputs changed" and never as an output change.

This is the record a "bit-identical" claim about the kernels is checked against.  A change that is meant to alter the arithmetic
regenerates the file on an MI355X and says so:

    python tests/test_gpu_family_bits.py --record"""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path[:0] = [str(Path(__file__).resolve().parent), str(Path(__file__).resolve().parents[1])]

from quality_mix import FAMILIES, TABLES, family_problem, run_with_env

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "family_bits.json"
QUALS = ("full", "edges", "max")
PILEUP_ARRAYS = ("cell_pair_off", "cell_read_off", "pair_snp", "pair_nrd", "reads", "rd_totl", "rd_pass", "rd_uniq")


def digest(arrays):
    """SHA-256 over (name, dtype, shape, bytes) of each array, in order; None hashes as its name alone."""
    h = hashlib.sha256()
    for name, a in arrays:
        h.update(name.encode())
        if a is not None:
            a = np.ascontiguousarray(a)
            h.update(f"{a.dtype.str}{a.shape}".encode())
            h.update(a.tobytes())
    return h.hexdigest()


def input_digest(g, sp):
    return digest([("g", g)] + [(n, getattr(sp, n)) for n in PILEUP_ARRAYS])


def output_digest(out):
    summ = out["summ"]
    return digest([(n, out[n]) for n in ("llks", "llk0s", "grid", "l00")] + [(n, summ[n]) for n in summ.dtype.names])


@pytest.fixture(scope="module")
def eng():
    from demuxlet_amd import build, capi, engine
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return engine


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.mark.parametrize("quals", QUALS)
@pytest.mark.parametrize("case,field,V,alphas,mode,env,k1,k2,dense,deep", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_kernel_family_bits(eng, golden, monkeypatch, case, field, V, alphas, mode, env, k1, k2, dense, deep, quals):
    want = golden[f"{case}/{quals}"]
    g, sp = family_problem(eng, case, field, V, dense, deep, quals)
    assert input_digest(g, sp) == want["inputs"], "inputs changed: regenerate"
    got = {}
    for tname, tenv in TABLES.items():
        out = run_with_env(eng, monkeypatch, g, sp, alphas, mode, {**env, **tenv})
        names = out["names"]
        assert names["singlet"].startswith(k1) and names["doublet"].startswith(k2), (tname, names)
        got[tname] = output_digest(out)
    assert got == {t: want[t] for t in TABLES}


def record():
    from demuxlet_amd import build, capi, engine
    build.build()
    capi.load()
    rec = {}
    with pytest.MonkeyPatch.context() as mp:
        for case, field, V, alphas, mode, env, k1, k2, dense, deep in FAMILIES:
            for quals in QUALS:
                g, sp = family_problem(engine, case, field, V, dense, deep, quals)
                r = rec[f"{case}/{quals}"] = {"inputs": input_digest(g, sp)}
                for tname, tenv in TABLES.items():
                    out = run_with_env(engine, mp, g, sp, alphas, mode, {**env, **tenv})
                    assert out["names"]["singlet"].startswith(k1) and out["names"]["doublet"].startswith(k2), (case, tname, out["names"])
                    r[tname] = output_digest(out)
    return rec


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], "usage: python tests/test_gpu_family_bits.py --record [out.json]"
    dst = Path(sys.argv[2]) if len(sys.argv) > 2 else GOLDEN
    dst.parent.mkdir(parents=True, exist_ok=True)
    dst.write_text(json.dumps(record(), indent=1, sort_keys=True) + "\n")
    print(f"recorded {dst}")
