"""lvl_linear_wgrad's tile configurations as the tests see them: the plan query (lvl_linear_wgrad_plan: the launch's own
make_plan / row_plan), the kernel's block decode (lvl_linear_wgrad_pair_of_block), the precondition of the late-workgroup
hook, and the case table shared by test_wgrad_plan_cpu.py (every row reaches its configuration, on the CPU) and
test_gpu_wgrad_configs.py (every row runs on every schedule)."""
import collections
import contextlib
import ctypes

# workgroup shapes {WN, WK, TA, TB} of csrc/wgrad_mfma.hip (tile = 16*TA*WN x 16*TB*WK); from FIRST_160 on: the 160 family
CFGS = ((4, 2, 6, 6), (2, 4, 6, 6), (3, 2, 6, 6), (2, 3, 6, 6), (2, 2, 6, 6), (2, 4, 8, 4), (2, 2, 8, 4), (1, 4, 8, 4),
        (4, 2, 5, 5), (2, 4, 5, 5), (2, 2, 5, 5), (2, 4, 8, 5), (2, 2, 8, 5))
FIRST_160 = 8
FIELDS = ('cfg', 'tiles_k', 'ntiles', 'S', 'base', 'rem', 'L', 'nch0', 'nch1')
ENOSYS = -38
COUNTER_WORDS = 1024          # the chunk-counter block ops.sched_block hands to a launch
LATE_MODS = (1024, 3)         # lvl_debug_late_workgroups settings: only block 1 late / every third block late


@contextlib.contextmanager
def compute_units(lib, cus):
    """lvl_set_compute_units(cus) (0 = the device's own) for the plans and launches inside; reset in any case"""
    try:
        assert lib.lvl_set_compute_units(cus) == 0
        yield
    finally:
        assert lib.lvl_set_compute_units(0) == 0


def plan(lib, M, N, K):
    """dict of FIELDS for what lvl_linear_wgrad launches at (M, N, K) under the current CU limit (M = 0: the workspace
    plan); None where the library has no tiling"""
    out = (ctypes.c_int * len(FIELDS))(*([-1] * len(FIELDS)))
    rc = lib.lvl_linear_wgrad_plan(M, N, K, out)
    if rc == ENOSYS:
        return None
    assert rc == 0, (rc, lib.lvl_last_error())
    return dict(zip(FIELDS, out))


def chunks(p):
    """chunks per unit of the dynamic schedule: the largest over the units that exist"""
    return p['nch1'] if p['rem'] else p['nch0']


def tile_of_block(lib, p, bid):
    return lib.lvl_linear_wgrad_pair_of_block(p['cfg'], p['ntiles'] * p['S'], bid) % p['ntiles']


def late_ok(lib, p, late_mod):
    """The precondition of the late hook (workgroups with bid % late_mod == 1 visit nothing): every tile keeps at least
    one split whose workgroup is not late -- a tile whose S workgroups are all late is computed by nobody."""
    alive = [0] * p['ntiles']
    for bid in range(p['ntiles'] * p['S']):
        if bid % late_mod != 1:
            alive[tile_of_block(lib, p, bid)] += 1
    return min(alive) >= 1


def late_mods(lib, p):
    """the late settings a launch of plan p may run with"""
    return tuple(m for m in LATE_MODS if p['S'] >= 2 and late_ok(lib, p, m))


# One row: configuration `cfg` is what the library plans for (M, N, K) at `cus` compute units (0 = the device's own: the
# 256 of an MI355X, which is also what the library assumes without a device).
#   'one'   a one-chunk static case at the device's CU count
#   'multi' S >= 2 splits and >= 3 chunks per unit at 8 CUs: chunk boundaries crossed, tile-mates to steal from
# M is a multiple of 32; the GPU test runs M, M + 1 and M + 31 (same plan: the tail rows go to the reduction kernel).
Case = collections.namedtuple('Case', 'cfg kind N K M cus')
CASES = (
    Case(0, 'one', 384, 192, 1536, 0), Case(1, 'one', 192, 384, 1536, 0), Case(2, 'one', 288, 192, 1536, 0),
    Case(3, 'one', 192, 288, 1536, 0), Case(4, 'one', 192, 192, 1536, 0), Case(5, 'one', 256, 256, 1536, 0),
    Case(6, 'one', 256, 128, 1536, 0), Case(7, 'one', 128, 256, 1536, 0),
    # the 160 family is planned only where no older configuration divides the shape: 130 tiles of 320 x 160 / 160 x 320
    # and 72 of 256 x 320 are the smallest shapes on which the 8-wave configurations win at 256 CUs
    Case(8, 'one', 3200, 2080, 1536, 0), Case(9, 'one', 2080, 3200, 1536, 0), Case(10, 'one', 160, 160, 1536, 0),
    Case(11, 'one', 2048, 2880, 3072, 0), Case(12, 'one', 256, 160, 1536, 0),
    # 2 tiles x 4 splits (cfg 4: 1 x 8), units of 150 row blocks in chunks of 52, 52, 46 (cfg 4: units of 156 and 157 blocks:
    # the odd last chunk)
    Case(0, 'multi', 384, 384, 19200, 8), Case(1, 'multi', 192, 768, 19200, 8), Case(2, 'multi', 288, 384, 19200, 8),
    Case(3, 'multi', 192, 576, 19200, 8), Case(4, 'multi', 192, 192, 40000, 8), Case(5, 'multi', 256, 512, 19200, 8),
    Case(6, 'multi', 512, 128, 19200, 8), Case(7, 'multi', 128, 512, 19200, 8),
    # 3 tiles x 2 splits: 6 pairs, not a multiple of 8 (blocks 1 and 4 share tile 1: no late_mod = 3 here)
    Case(8, 'multi', 320, 480, 9600, 8), Case(9, 'multi', 160, 960, 9600, 8), Case(10, 'multi', 160, 480, 9600, 8),
    Case(11, 'multi', 256, 960, 9600, 8), Case(12, 'multi', 256, 480, 9600, 8),
    # the 160 family on 2 tiles x 4 splits and 1 tile x 8 splits, where every third workgroup may be late
    Case(8, 'multi', 320, 320, 19200, 8), Case(9, 'multi', 160, 640, 19200, 8), Case(11, 'multi', 256, 320, 38400, 8),
)
REMAINDERS = (0, 1, 31)


def case_id(c):
    return f'cfg{c.cfg}-{c.kind}-{c.N}x{c.K}-M{c.M}-cus{c.cus}'
