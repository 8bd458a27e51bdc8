"""The LDS a rupture-time sweep launch asks for (beatamd_fast_sweep_lds, the rule of sweep.hip's launch_sweep): host only."""
import ctypes

import pytest

WG_DEFAULT = 64 * 1024     # dynamic LDS a launch gets without opting in
WG_MAX = 160 * 1024        # LDS of a compute unit of the MI355X
MAX_CELLS = 6400           # the limit of beatamd_fast_sweep_batch


def _plan(ncells):
    from beat_amd import _lib
    waves = ctypes.c_int32(0)
    nbytes = _lib.load().beatamd_fast_sweep_lds(ncells, ctypes.byref(waves))
    return nbytes, waves.value


def test_sweep_lds_stays_within_the_workgroup_limits():
    seen = set()
    for n in range(1, MAX_CELLS + 1):
        nbytes, waves = _plan(n)
        assert waves in (1, 4), n
        seen.add(waves)
        nmax = (n + 1) & ~1
        # t, told and the slowness area of every grid of the workgroup
        assert nbytes >= waves * 3 * nmax * 8, n
        assert nbytes % 16 == 0, n
        assert nbytes <= (WG_DEFAULT if waves == 4 else WG_MAX), (n, nbytes)
    assert seen == {1, 4}
    assert _plan(MAX_CELLS)[0] <= WG_MAX


def test_sweep_lds_of_the_shipped_subfaults():
    # the bench fault: four grids per workgroup, with their slowness terms (32 bytes per cell)
    assert _plan(400) == (4 * 32 * 400, 4)
    # the four-grid workgroup ends where its LDS would pass 64 KiB
    assert _plan(512) == (64 * 1024, 4)
    assert _plan(513) == (32 * 514, 1)
    # the largest grid that keeps slowness terms, and the first that runs the first version on three arrays
    assert _plan(5120) == (160 * 1024, 1)
    assert _plan(5121) == (24 * 5122, 1)


@pytest.mark.parametrize("n", [0, -1, MAX_CELLS + 1])
def test_sweep_lds_rejects_what_the_sweep_rejects(n):
    assert _plan(n)[0] == -1
