"""The exact receivers of the HIP library (LSDR_RX_SERIAL and lsdr_rx_batch, through the C ABI) on every constellation: BPSK 1/2,
QPSK 7/8, 8PSK 2/3, 16APSK 3/4, 32APSK 4/5, 64APSK 5/6, 16QAM 3/4, 64QAM 5/6 and 256QAM 7/8 at 1.2, 3, 4 and 8 samples per symbol
(tests/modcod_common.py), bit for bit against the oracle — which test_oracle_vs_ref.py / test_oracle_golden.py pin to the reference on
exactly these inputs.  What only dense tables reach: symbols >= 128 and points beyond +-63 in the packed table entry, the two-symbol
estimator branch, the per-constellation divisor of the frequency limits (the `clamp` variant) and the skip loop at omega 1.2, 3 and 8.
The serial receiver runs every setting; lsdr_rx_batch runs at 4 samples per symbol (the sps4 and clamp settings)."""
import numpy as np
import pytest
from conftest import gold, bits_equal
from test_oracle_golden import state_vec
import pyoracle as po
import modcod_common as mc

pytestmark = pytest.mark.gpu


def rrc_of(sampler):
    return gold("tables.npz")["rrc_rx"] if sampler == 2 else None


def same_symbols(got, want):
    assert len(got) == len(want)
    assert bits_equal(got["cost"], want["cost"]) and bits_equal(got["symbol"], want["symbol"])


def same_state(st, want):
    sv, mc_ = state_vec(st)
    wv, wc = state_vec(want)
    assert bits_equal(sv, wv) and mc_ == wc


@pytest.mark.parametrize("case", mc.RX_GPU, ids=mc.case_id)
def test_serial_vs_oracle(capi, ctx, oracle, case):
    c, r, v, s = case
    want = mc.oracle_rx(oracle, case, rrc_of(s))
    rx = capi.CstlnReceiver(ctx, mode=capi.RX_SERIAL, **mc.rx_kwargs(c, r, v, s, rrc_of(s)))
    out = rx.run(mc.rx_input(oracle, c, r, v, s), meas=True)
    rx.close()
    assert out["consumed"] == want["consumed"]
    same_symbols(out["sym"], want["sym"])
    for k in ("freq", "ss", "mer", "cstln"):
        assert bits_equal(out[k], want[k]), k
    same_state(out["state"], want["state"])


@pytest.mark.parametrize("case", [(8, 5, "sps4", 1), (4, 6, "sps1p2", 1)], ids=mc.case_id)
def test_streaming_dense_tables(capi, ctx, oracle, case):
    """The stream in uneven pieces through one handle == the oracle's one shot: symbols, measurements and the loop state."""
    c, r, v, s = case
    want = mc.oracle_rx(oracle, case)
    x = mc.capture(oracle, c, r, v)
    rx = capi.CstlnReceiver(ctx, mode=capi.RX_SERIAL, **mc.rx_kwargs(c, r, v, s))
    outs, pos = [], 0
    for piece in (5000, 129, 128, 100, 17000, 1 << 30):
        o = rx.run(x[pos:pos + piece], meas=True)
        outs.append(o)
        pos += o["consumed"]
    st = rx.state()
    rx.close()
    assert pos == want["consumed"]
    same_symbols(np.concatenate([o["sym"] for o in outs]), want["sym"])
    for k in ("freq", "ss", "mer", "cstln"):
        assert bits_equal(np.concatenate([o[k] for o in outs]), want[k]), k
    same_state(st, want["state"])


@pytest.mark.parametrize("case", [(3, 3, "sps4", 1), (8, 5, "sps4", 1)], ids=mc.case_id)
def test_harden(capi, ctx, oracle, case):
    """harden = 1 (cstln_lut::harden, sdr.h:564-571; the oracle's lo_cstln_harden) replaces every cost of the table by its sign and
    nothing else: the receiver's loops never read a cost, so symbols, measurements and state are the oracle's, and each soft symbol's
    cost is the sign of the oracle's."""
    c, r, v, s = case
    want = mc.oracle_rx(oracle, case)
    rx = capi.CstlnReceiver(ctx, mode=capi.RX_SERIAL, harden=1, **mc.rx_kwargs(c, r, v, s))
    out = rx.run(mc.rx_input(oracle, c, r, v, s), meas=True)
    rx.close()
    assert out["consumed"] == want["consumed"] and bits_equal(out["sym"]["symbol"], want["sym"]["symbol"])
    wc = want["sym"]["cost"]
    assert np.abs(wc.astype(np.int32)).max() > 1          # (the plain costs are not their own signs)
    assert bits_equal(out["sym"]["cost"], np.sign(wc).astype(wc.dtype))
    for k in ("freq", "ss", "mer", "cstln"):
        assert bits_equal(out[k], want[k]), k
    same_state(out["state"], want["state"])


@pytest.mark.parametrize("setting", ["sps4", "clamp"])
@pytest.mark.parametrize("sampler", [0, 1])
@pytest.mark.parametrize("cstln,rate", mc.MODCODS)
def test_batch_lane_per_capture(capi, ctx, oracle, cstln, rate, sampler, setting):
    """lsdr_rx_batch on every constellation: 6 captures (the sps4 and the clamp signal under three noise seeds each), two consecutive
    runs, once with the sps4 receiver setting and once with the clamp one, whose loop gain drives the frequency word into its limits:
    each capture's soft symbols and the seven float state fields are the oracle's."""
    n = 128 * 70 + 1
    xs = [mc.capture(oracle, cstln, rate, v, seed=1000 * k + cstln * 16 + rate)[:2 * n] for v in ("sps4", "clamp") for k in (1, 2, 3)]
    assert all(len(x) == 2 * n for x in xs)
    kw = mc.rx_kwargs(cstln, rate, setting, sampler)
    b = capi.RxBatch(ctx, len(xs), **kw)
    d_in = [ctx.upload(x) for x in xs]
    d_out = [ctx.alloc(2 * n * 4) for _ in xs]
    got = [[] for _ in xs]
    pos = 0
    for _ in range(2):
        cons, prod = b.run_dev([d.at(pos * 8) for d in d_in], n, [d.ptr for d in d_out], 2 * n)
        assert cons == (n - (1 if sampler else 0)) // 128 * 128
        for i in range(len(xs)):
            got[i].append(ctx.download(d_out[i], capi.SOFTSYM, prod[i]).copy())
        pos += cons
    states = [b.state(i) for i in range(len(xs))]
    b.close()
    for d in d_in + d_out:
        d.free()
    for i, x in enumerate(xs):
        want = oracle.rx(po.rx_params(**kw), x[:pos + (1 if sampler else 0)])
        assert want["consumed"] == pos, i
        same_symbols(np.concatenate(got[i]), want["sym"])
        for k in ("mu", "phase", "freqw", "agc_gain", "est_insp", "est_sp", "est_ep"):
            assert np.float32(getattr(states[i], k)).tobytes() == np.float32(getattr(want["state"], k)).tobytes(), (i, k)
