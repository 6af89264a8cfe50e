"""oracle/_ref - the reference's own C for the DF J/K hot path (pyscf/lib/ao2mo/nr_ao2mo.c:399-419,1016-1031,1240-1266 and
pyscf/lib/np_helper/{pack_tril,npdot}.c, compiled in place by `make -C oracle ref`) - against the numpy restatement in
oracle/ref.py and against the reference's golden fingerprints.  This is what bench.py's cpu_baseline (kind "reference") times.

oracle/_ref can only be built where the reference's sources are.  What it returns on the cases below is stored in
tests/golden/ref_c_h2o_dz.npz (tools/gen_golden_ref_c.py): without the library the restatement is checked against that copy,
with it the library is run as well and must reproduce the copy."""
import os

import numpy as np
import pytest

from oracle import ref, ref_c
from pyscf_amd import gto, df
from tests.conftest import H2O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_c_h2o_dz.npz')
LIVE = ref_c.build()
BLOCKS = (240, 50, 7)                                                # several blocks, ragged last block


def _case(basis='cc-pvdz', aux='weigend', seed=3):
    mol = gto.M(atom=H2O, basis=basis)
    cderi = ref.cholesky_eri(mol, df.make_auxmol(mol, aux))
    nao, nocc = mol.nao, mol.nelectron // 2
    c = np.linalg.qr(np.random.RandomState(seed).rand(nao, nao))[0]
    occ = np.zeros(nao)
    occ[:nocc] = 2
    return mol, cderi, c, occ, (c[:, :nocc] * 2).dot(c[:, :nocc].T)


def _pack_inputs():
    rng = np.random.RandomState(0)
    a = rng.rand(3, 9, 9)
    a = a + a.transpose(0, 2, 1)
    return a, [rng.rand(k, n) for k, n in ((400, 5), (7, 11))]          # both NPdgemm strategies (parallel over k / plain)


def reference_outputs():
    """What oracle/_ref returns on this module's cases (the dict tools/gen_golden_ref_c.py stores)."""
    mol, cderi, c, occ, dm = _case()
    out = {}
    for blk in BLOCKS:
        out['vj_blk%d' % blk], out['vk_blk%d' % blk], _ = ref_c.get_jk(cderi, dm, c, occ, blockdim=blk, nthreads=2)
    out['vj_default'], out['vk_default'], _ = ref_c.get_jk(cderi, dm, c, occ)
    a, bs = _pack_inputs()
    out['pack_tril'] = ref_c.pack_tril(a)
    out['unpack_tril'] = ref_c.unpack_tril(out['pack_tril'])
    for i, b in enumerate(bs):
        out['dot_tn_%d' % i] = ref_c.lib_dot_tn(b)
    return out


@pytest.fixture(scope='module')
def reference():
    """oracle/_ref's outputs: run now where the library is built (and equal to the stored copy), else the stored copy."""
    with np.load(GOLDEN) as z:
        stored = {k: z[k] for k in z.files}
    if not LIVE:
        return stored
    live = reference_outputs()
    assert sorted(live) == sorted(stored)
    for k, v in live.items():
        assert v.shape == stored[k].shape and np.abs(v - stored[k]).max() <= 1e-12 * max(1.0, np.abs(v).max()), k
    return live


def test_reference_c_jk_equals_restatement(reference):
    mol, cderi, c, occ, dm = _case()
    vj0, vk0 = ref.get_jk(cderi, dm, hermi=1)                         # general-DM branch of the restatement
    for blk in BLOCKS:
        vj, vk = reference['vj_blk%d' % blk], reference['vk_blk%d' % blk]
        assert np.abs(vj - vj0).max() < 1e-12 and np.abs(vk - vk0).max() < 1e-12
    if LIVE:                                                         # the driver's own bookkeeping
        flops = ref_c.get_jk(cderi, dm, c, occ, blockdim=BLOCKS[-1], nthreads=2)[2]
        assert flops > 0 and set(ref_c.get_jk.last_phases) == {'pack', 'vj', 'e2_drv', 'dot', 'unpack'}


def test_reference_c_pack_unpack_and_npdgemm(reference):
    a, bs = _pack_inputs()
    t = reference['pack_tril']
    assert np.array_equal(t, ref.pack_tril(a)) and np.array_equal(reference['unpack_tril'], a)
    for i, b in enumerate(bs):
        assert np.abs(reference['dot_tn_%d' % i] - b.T.dot(b)).max() < 1e-12


def test_reference_c_reproduces_golden_energy_ingredients(reference):
    """E(DF-RHF) of the reference's test_df_jk.py:57-59 is built from these J/K: the _ref path must give the restatement's
    converged energy ingredients at the converged density."""
    mol, cderi, c, occ, dm = _case(aux='weigend')
    vj, vk = reference['vj_default'], reference['vk_default']
    vj0, vk0 = ref.get_jk(cderi, dm, hermi=1)
    assert abs(np.einsum('ij,ji', dm, vj - .5 * vk) - np.einsum('ij,ji', dm, vj0 - .5 * vk0)) < 1e-11
