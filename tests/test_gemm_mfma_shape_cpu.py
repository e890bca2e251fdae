"""Host-only, from the gfx950 ISA: the v_mfma_f32_16x16x32_bf16 instantiations of the persistent TN GEMM (gemm_tn_mfma16<EPI>
in csrc/gemm_tn_kernel.h, instantiated by csrc/gemm_tn_mfma.hip for the bf16 epilogues 0-5) meet what
test_boundary_cpu.test_gemm_tile_counter_reply_register_is_untouched_in_isa asks of the 32x32x16 ones, their K loop holds
the MFMAs it should, and the ten 32x32x16 instantiations are still what they were."""
import re

import pytest

from test_boundary_cpu import _check_parked_reply_registers, _isa, _kernel_bodies

K_BLOCK_COPIES = 3        # k_block(IS, IS), k_block(IS, I0), k_block(I0, I0): the text of one K block, three times per kernel


@pytest.fixture(scope='module')
def isa(tmp_path_factory):
    d = tmp_path_factory.mktemp('gemm_mfma_shape_isa')
    return _isa(d, 'gemm_tn_mfma'), _isa(d, 'gemm_tn_mfma', defines=('GM_AUDIT',))


def _phases(body):
    """MFMA mnemonics between consecutive s_barrier instructions (the stretches that hold any)"""
    out, cur = [], []
    for l in body:
        if l.startswith('s_barrier'):
            if cur:
                out.append(cur)
            cur = []
        elif l.startswith('v_mfma'):
            cur.append(l.split()[0])
    return out + ([cur] if cur else [])


def test_mfma16_instantiations_in_the_isa(isa):
    """six kernels (epilogues 0-5), under a symbol that does not contain the stem the other tests count; no scratch access
    between the first and the last MFMA; the tile-counter reply register untouched while the reply is in flight (3
    requests); the tile loop holds v_mfma_f32_16x16x32_bf16 only: 64 per K block per wave (4 phases of 16 between bare
    barriers)"""
    product, _ = isa
    bodies = list(_kernel_bodies(product, 'gemm_tn_mfma16'))
    assert sorted(re.search(r'gemm_tn_mfma16ILi(\d)E', n).group(1) for n, _ in bodies) == list('012345')
    for name, body in bodies:
        assert 'gemm_tn_kernel' not in name
        mf = [i for i, l in enumerate(body) if l.startswith('v_mfma')]
        assert not any('scratch_' in l for l in body[mf[0]:mf[-1]]), f'VGPR spills inside the tile loop of {name}'
        _check_parked_reply_registers(name, body, 3)
        assert {body[i].split()[0] for i in mf} == {'v_mfma_f32_16x16x32_bf16'}, name
        assert len(mf) == K_BLOCK_COPIES * 64, (name, len(mf))
        phases = _phases(body)
        assert len(phases) == K_BLOCK_COPIES * 4 and all(len(p) == 16 for p in phases), (name, [len(p) for p in phases])


def test_mfma16_instantiations_of_the_audit_build_have_no_private_segment(isa):
    """GM_AUDIT build: the bookkeeping adds no vector-memory operation of its own -- no private segment, no VGPR spill"""
    _, audit = isa
    meta = {}
    for l in audit:
        m = re.match(r'\s+\.(name|private_segment_fixed_size|vgpr_spill_count):\s+(\S+)', l)
        if m and m.group(1) == 'name':
            cur = meta.setdefault(m.group(2), {})
        elif m:
            cur[m.group(1)] = int(m.group(2))
    meta = {k: v for k, v in meta.items() if 'gemm_tn_mfma16' in k}
    assert len(meta) == 6
    for name, v in meta.items():
        assert v == {'private_segment_fixed_size': 0, 'vgpr_spill_count': 0}, (name, v)


def test_the_32x32x16_instantiations_are_what_they_were(isa):
    """ten kernels under the old stem (6 bf16 epilogues + 4 f32-class ones), v_mfma_f32_32x32x16_bf16 only: 32 per K block
    per wave, 4 phases of 8"""
    product, _ = isa
    bodies = list(_kernel_bodies(product, 'gemm_tn_kernel'))
    assert len(bodies) == 10
    assert sum('Lb1E' in n for n, _ in bodies) == 4
    for name, body in bodies:
        mf = [l.split()[0] for l in body if l.startswith('v_mfma')]
        assert set(mf) == {'v_mfma_f32_32x32x16_bf16'} and len(mf) == K_BLOCK_COPIES * 32, (name, len(mf))
        phases = _phases(body)
        assert len(phases) == K_BLOCK_COPIES * 4 and all(len(p) == 8 for p in phases), (name, [len(p) for p in phases])
