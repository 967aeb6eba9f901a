"""The exit gate's threshold (DecodeArgs::exit_gate) is a
diagnostic knob like the others: read through the library's diagnostic switch
only.  No GPU here: qldpc_exit_gate() answers what a launch would be handed."""
import qkd_ldpc_v_amd as Q


def gate():
    return int(Q.lib().qldpc_exit_gate())


def test_exit_gate_ignored_without_diag_switch(monkeypatch):
    monkeypatch.delenv("QLDPC_DIAG", raising=False)
    monkeypatch.delenv("QLDPC_EXIT_GATE", raising=False)
    default = gate()
    assert default >= 0  # the product runs the pass
    for v in ("-1", "0", "7", str(2**31 - 1)):
        monkeypatch.setenv("QLDPC_EXIT_GATE", v)
        assert gate() == default, v
    monkeypatch.setenv("QLDPC_DIAG", "0")  # only "1" switches the knobs on
    assert gate() == default


def test_exit_gate_acts_under_diag_switch(monkeypatch):
    monkeypatch.delenv("QLDPC_EXIT_GATE", raising=False)
    monkeypatch.setenv("QLDPC_DIAG", "1")
    default = gate()
    for v in (-1, 0, 7, 2**31 - 1):
        monkeypatch.setenv("QLDPC_EXIT_GATE", str(v))
        assert gate() == v
    monkeypatch.setenv("QLDPC_EXIT_GATE", "")  # empty: the default, as for every knob
    assert gate() == default
