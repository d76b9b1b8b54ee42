"""The host's plan of a pass over resident posterior samples (dynetlsm_amd/csrc/pass_plan.hpp: the tiles of a time
step, the tiles per workgroup and workgroups per time step, the byte accounting of a pass's buffer list) checked
without a GPU: for N in {2, 3, 31, 32, 33, 63, 64, 65, 96, 129, 200}, tile heights {1, 2, 4, 16, 32} and both models
every dyad lies in exactly one listed tile, in row-block-major order; the grid covers the tiles within its cap; the
memory budget is the sum of the declared buffers and the outputs come back in the order of their declaration - under
ASan / UBSan."""
import os

from test_sanitizers_cpu import ROOT, _build_and_run


def test_pass_plan_tiles_grid_and_buffers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'native', 'check_pass_plan.cpp')
    out = _build_and_run(tmp_path, 'g++', [src], extra=['-std=c++17'])
    assert 'check_pass_plan ok' in out
