"""The packed workspaces' layouts (dynetlsm_amd/csrc/workspace.hpp: the sweeps' buffers, the HDP-LPCM loop's
auxiliary buffers, the case-control pass's gather records) checked without a GPU: for T in {1, 2, 3}, N in {2, 3, 127,
128, 129, 513}, d in {1, 3, 8}, K in {1, 5} and 0, 1 or 7 terms per node the sizing run equals the closed-form total
the launchers used to spell out, the regions follow each other without overlap, aligned to their element type (16 bytes
where a kernel reads double2), the last one ends at the total, and the carving run over a host allocation of that total
writes the first and last element of every region - under ASan / UBSan."""
import os

from test_sanitizers_cpu import ROOT, _build_and_run


def test_workspace_layouts_size_order_alignment_and_bounds(tmp_path):
    src = os.path.join(ROOT, 'tests', 'native', 'check_workspace.cpp')
    out = _build_and_run(tmp_path, 'g++', [src], extra=['-std=c++17'])
    assert 'check_workspace ok' in out
