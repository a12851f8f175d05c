"""The two configurations of the shared symbol walk (symbolsync.Walker): what qpsk.Walker and bpsk.Walker state, read without a GPU,
so that neither decoder can end up with the other's symbol rate, loop bandwidth, AGC start, lim width or entry points."""
import numpy as np

from directdemod_amd import bpsk, qpsk, symbolsync


def test_walker_configurations():
    q, b = qpsk.Walker, bpsk.Walker
    assert (q.SYMBOL_RATE, b.SYMBOL_RATE) == (72000, 12000) == (qpsk.SYMBOL_RATE, bpsk.SYMBOL_RATE)
    assert (q.AMEAN0, b.AMEAN0) == (3.0, 180.0)
    assert (np.dtype(q.LIM_DTYPE), np.dtype(b.LIM_DTYPE)) == (np.dtype(np.int16), np.dtype(np.int8))
    assert (q.WALK, q.LIM, q.LABEL) == ("dd_meteor_walk", "dd_meteor_lim", "meteor")
    assert (b.WALK, b.LIM, b.LABEL) == ("dd_funcube_walk", "dd_funcube_lim", "funcube")
    assert symbolsync.costas_coefficients(q.COSTAS_BW) == qpsk.costas_coefficients()
    assert symbolsync.costas_coefficients(b.COSTAS_BW) == bpsk.costas_coefficients()
    assert qpsk.costas_coefficients() != bpsk.costas_coefficients()
    fs = 2048000
    for w, rate, coef in ((q, 72000, qpsk.costas_coefficients()), (b, 12000, bpsk.costas_coefficients())):
        P = fs / rate
        lead = w.leading_params(fs)
        assert lead == [P, P / 2, (P / 2) + 1] + list(coef) and all(type(v) is float for v in lead)
    for name in ("__init__", "walk", "lim", "view"):
        assert getattr(q, name) is getattr(b, name) is getattr(symbolsync.Walker, name)
    assert qpsk._STATE is symbolsync._STATE and qpsk._STATE.itemsize == 17 * 8
    assert qpsk.lim is bpsk.lim is symbolsync.lim and qpsk.limBin is bpsk.limBin and qpsk.mix is bpsk.mix
