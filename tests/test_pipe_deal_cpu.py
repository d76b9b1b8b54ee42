"""The pipelined sweep's deal (dynetlsm_amd/csrc/pipe_plan.hpp: which item a wavefront of an evaluator workgroup
takes, at 16 or - in the head launch - at 8 nodes per workgroup) checked without a GPU: for T in 1..12, N in {512,
520, 640, 2000, 2100}, 64..304 CUs and every launch, every (slice, part, node) item is owned by exactly one
(workgroup, wavefront) under the kernel's decode, the workgroups fit, and a launch whose resolvers have work keeps 16
nodes per workgroup - under ASan / UBSan."""
import os

from test_sanitizers_cpu import ROOT, _build_and_run


def test_pipe_deal_owns_every_item_once(tmp_path):
    src = os.path.join(ROOT, 'tests', 'native', 'check_pipe_deal.cpp')
    out = _build_and_run(tmp_path, 'g++', [src], extra=['-std=c++17'])
    assert 'check_pipe_deal ok' in out
