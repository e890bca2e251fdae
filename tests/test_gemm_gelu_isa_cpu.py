"""CPU (-m "not gpu"): the gfx950 ISA of csrc/gemm_tn_gelu.hip, the translation unit of lvl_linear_tn's exact-GELU epilogues
(6, 7, 8 in bf16; 6, 7 in f32-class mode), held to what tests/test_boundary_cpu.py holds the instantiations of
csrc/gemm_tn_mfma.hip to: no scratch at all (the erf must not cost a spill: a reload is a vector-memory operation the counted
vmcnt waits do not know), the parked reply of the tile-counter atomic untouched between its request and its publish, and a
GM_AUDIT build that adds no private segment and no VGPR spill of its own. gemm_tn_mfma.hip itself keeps exactly its ten
instantiations."""
import re

from test_boundary_cpu import _check_parked_reply_registers, _isa, _kernel_bodies


def test_gelu_instantiations_have_no_scratch_and_keep_the_parked_reply(tmp_path):
    lines = _isa(tmp_path, 'gemm_tn_gelu')
    bodies = list(_kernel_bodies(lines, 'gemm_tn_kernel'))
    assert sorted(re.search(r'ILi(\d)ELb(\d)', n).groups() for n, _ in bodies) == \
        [('6', '0'), ('6', '1'), ('7', '0'), ('7', '1'), ('8', '0')]
    for name, body in bodies:
        assert not any('scratch_' in l for l in body), f'scratch traffic in {name}'
        _check_parked_reply_registers(name, body, 3)           # first hand-out, tile 1, the per-tile pull
    for defines in ((), ('GM_AUDIT',)):
        meta = {}
        for l in _isa(tmp_path, 'gemm_tn_gelu', defines=defines):
            m = re.match(r'\s+\.(name|private_segment_fixed_size|vgpr_spill_count):\s+(\S+)', l)
            if m and m.group(1) == 'name':
                cur = meta.setdefault(m.group(2), {})
            elif m:
                cur[m.group(1)] = int(m.group(2))
        meta = {k: v for k, v in meta.items() if 'gemm_tn_kernel' in k}
        assert len(meta) == 5
        for name, v in meta.items():
            assert v == {'private_segment_fixed_size': 0, 'vgpr_spill_count': 0}, (defines, name, v)
    # the unit of the earlier epilogues holds no GELU instantiation
    names = [n for n, _ in _kernel_bodies(_isa(tmp_path, 'gemm_tn_mfma'), 'gemm_tn_kernel')]
    assert len(names) == 10 and not any(re.search(r'ILi[678]E', n) for n in names)
