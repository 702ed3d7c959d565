"""GPU: the resident kernel instances with the optimiser compiled in (k_res / k_stream<.., OS = true>, bb_opt_apply<0, 0>) against the
generic instances of the same shapes -- the BASELINE workloads' instances on cuts of their problems with the full-size tile geometry
(tests/_cases.py, BASELINE_INSTANCES).  Two handles in one process, the second created with BB_TUNE_OPT_SPEC=0: the same steps on the same
numbers, so parameters, accumulators and the window sums' low-order parts agree bit for bit; bb_stats.opt_compiled tells the forms
apart, bb_kernel_name does not."""
import numpy as np
import pytest

import _cases as c
from conftest import make_engine
from oracle import fixtures

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cfg", ["C2_fitness", "C3_replicate", "C4_multienv", "C5_rank", "C5_stream"])
def test_specialised_equals_generic(hip_lib, monkeypatch, cfg):
    """10 steps with a window of 4 slots (from step 4 on the slot that leaves the window is non-zero: the subtraction of the
    compensated sum), in two launches."""
    (kind, skw), nb, nthr, inst, env, _ = c.BASELINE_INSTANCES[cfg]
    sp = fixtures.synthetic(kind, **skw)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("BB_TUNE_NB", str(nb))
    monkeypatch.setenv("BB_TUNE_NTHR", str(nthr))
    outs = []
    for spec in (None, "0"):
        if spec is None:
            monkeypatch.delenv("BB_TUNE_OPT_SPEC", raising=False)
        else:
            monkeypatch.setenv("BB_TUNE_OPT_SPEC", spec)
        with make_engine(sp, hip_lib, seed=13, window=4, launch_mode=2) as e:
            st = e.stats()
            assert e.kernel_name() == inst, e.kernel_name()
            assert st["resident_kernel"] == (3 if cfg == "C5_stream" else 2) and st["block_threads"] == nthr, st
            assert st["opt_compiled"] == (1 if spec is None else 0), st
            e.run(4)
            e.run(6)
            assert e.stats()["steps_done"] == 10
            mu, om = e.get_params()
            outs.append((mu, om) + e.opt_state())
    assert np.all(np.isfinite(outs[0][0])) and np.all(np.isfinite(outs[0][1])) and np.any(outs[0][4] != 0.0)
    for x, y, what in zip(outs[0], outs[1], ("mu", "omega", "acc_mu", "acc_omega", "lo")):
        assert x.tobytes() == y.tobytes(), (what, int((x != y).sum()), float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()))


@pytest.mark.parametrize("kw", [dict(resum_every=1), dict(resum_every=3), dict(optimizer="DecayedADAGrad"), dict(elbo_every=1)],
                         ids=["resum_every_1", "resum_every_3", "DecayedADAGrad", "elbo_trace"])
def test_other_configurations_keep_the_generic_instance(hip_lib, monkeypatch, kw):
    (kind, skw), nb, nthr, inst, _, _ = c.BASELINE_INSTANCES["C2_fitness"]
    monkeypatch.setenv("BB_TUNE_NB", str(nb))
    monkeypatch.setenv("BB_TUNE_NTHR", str(nthr))
    with make_engine(fixtures.synthetic(kind, **skw), hip_lib, seed=13, window=4, launch_mode=2, **kw) as e:
        st = e.stats()
        assert st["resident_kernel"] == 2 and st["opt_compiled"] == 0, st
        e.run(5)
        assert np.all(np.isfinite(e.get_params()[0]))
