"""chain_common.h: xcd_tile_range -- the tile walk of the persistent chain kernels (bneck, l3_chain, res_chain) -- probed on the host (a tiny
program compiled with hipcc; nothing runs on a device): over every grid size and tile count the workgroups' walks together visit every tile
exactly once, in the XCD order (each XCD's workgroups share one contiguous eighth) when both counts are multiples of 8 and in the plain stride
otherwise."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBLK = (1, 7, 8, 16, 256)
NTILES = (1, 5, 8, 64, 300, 1024)


@pytest.fixture(scope='module')
def walks(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    exe = str(tmp_path_factory.mktemp('xcd') / 'xcd_tile_range_host')
    b = subprocess.run([hipcc, '--offload-arch=gfx950', '-O1', '-std=c++20', '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'dir_amd', 'csrc'),
                        '-o', exe, os.path.join(ROOT, 'tests', 'helpers', 'xcd_tile_range_host.hip')], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    cases = [(nblk, ntiles) for nblk in NBLK for ntiles in NTILES]
    r = subprocess.run([exe], input=''.join('%d %d\n' % c for c in cases), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == sum(nblk for nblk, _ in cases)
    out, pos = {}, 0
    for nblk, ntiles in cases:
        out[(nblk, ntiles)] = rows[pos:pos + nblk]
        pos += nblk
    return out


@pytest.mark.parametrize('nblk', NBLK)
@pytest.mark.parametrize('ntiles', NTILES)
def test_every_tile_is_visited_exactly_once(walks, nblk, ntiles):
    seen = [0] * ntiles
    for t0, tstep, tend in walks[(nblk, ntiles)]:
        assert t0 >= 0 and tstep >= 1 and tend <= ntiles
        for t in range(t0, tend, tstep):
            seen[t] += 1
    assert seen == [1] * ntiles


def test_both_orders_are_taken(walks):
    taken = set()
    for (nblk, ntiles), rows in walks.items():
        xcd = nblk % 8 == 0 and ntiles % 8 == 0
        taken.add(xcd)
        for bid, (t0, tstep, tend) in enumerate(rows):
            if xcd:          # XCD bid % 8 owns tiles [per * (bid % 8), per * (bid % 8 + 1)), its nblk / 8 workgroups interleaved
                per = ntiles // 8
                assert (t0, tstep, tend) == (per * (bid % 8) + bid // 8, nblk // 8, per * (bid % 8 + 1))
            else:
                assert (t0, tstep, tend) == (bid, nblk, ntiles)
    assert taken == {True, False}
