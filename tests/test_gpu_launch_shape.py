"""The one refusal of the launch path: rows partly in global scratch without
the bit gather (capi.hip decode_on, QLDPC_EUNSUP), on the device.

The graph is tests/test_gpu_shapes.py's hybrid_dv4_global (built once, shared
with that module); tests/test_launch_shape.py pins its shapes on the CPU.
"""
import pytest

import qkd_ldpc_v_amd as Q
from qkd_ldpc_v_amd._lib import QLDPCError
from test_gpu_parity import frames
from test_gpu_shapes import CAP, OMSA, SPA, assert_parity, bsc_parity, graph, matrix, qber

pytestmark = pytest.mark.gpu

CASE = "hybrid_dv4_global"


def test_rows_partly_global_need_the_bit_gather(gpu_available, monkeypatch):
    """Rows partly in global scratch exist for the bit gather alone: with
    QLDPC_VNG=0 (read per launch) a min-sum decode is refused with EUNSUP, SPA
    (rows in LDS) still decodes, and the same graph object decodes OMSA
    bitwise equal to the oracle again once the knob is gone."""
    alg, prim, sec = OMSA
    g = graph(CASE)
    _, _, llr, synd = frames(matrix(CASE), qber(CASE, alg), 2, 1)
    monkeypatch.setenv("QLDPC_DIAG", "1")
    monkeypatch.setenv("QLDPC_VNG", "0")
    with pytest.raises(QLDPCError) as e:
        g.decode(Q.Params(alg, CAP, True, 100.0, prim, sec), llr, synd, posterior=True)
    assert e.value.code == -5 and "need the bit gather" in str(e.value), e.value
    bsc_parity(CASE, *SPA, 2, spread=False)
    monkeypatch.delenv("QLDPC_VNG")
    assert graph(CASE) is g
    assert_parity(CASE, alg, prim, sec, llr, synd)
