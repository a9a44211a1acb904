"""CPU companion of tests/test_gpu_context_state.py: the orders, the references and the test's own logic, without a GPU.

  * the orders of every leg put every step first on a fresh context and behind every step it shares a cache key with, and the
    ordered pairs they promise cover context_sequences.REQUIRED -- the list leg i of the GPU module asserts on what it recorded;
  * every step's float64 reference is computable on the CPU (at N = 16 wherever one size does);
  * every leg's orders run on ONE numpy stand-in (tests/oracle_kernels.py, tests/helmholtz_kernels.py) wherever those
    implement the call: a kernel set without hidden state must pass in every order, so a failure here is the test's fault."""
import pytest

torch = pytest.importorskip("torch")

import context_sequences as cs  # noqa: E402


@pytest.fixture(scope="module")
def legs():
    out = cs.cpu_legs()
    for leg in out.values():
        leg.make_refs("cpu")
    yield out
    cs.release()


def test_orders_put_every_step_first_and_behind_every_step_it_shares_a_key_with():
    for legs in (cs.gpu_legs(), cs.cpu_legs()):
        for leg in legs.values():
            cs.check_orders(leg.steps, leg.orders)
    b = cs.gpu_legs()["b"]
    tags = [s.tag for s in b.steps]
    # 128 and 256 share the 128-point tables (z pass of 256, y and x passes of 128); no other two sizes of leg b share a length
    assert cs.fft_keys(128) & cs.fft_keys(256) == {("fft", 128)}
    sizes = cs.B_SIZES
    assert all(not (cs.fft_keys(m) & cs.fft_keys(n)) for m in sizes for n in sizes if m < n and (m, n) != (128, 256))
    assert [tags[i] for i in b.orders[0]] == ["spectrum %d" % n for n in cs.B_ORDER] + ["write %d" % n for n in cs.B_ORDER]


def test_promised_transitions_cover_the_required_list():
    recorded = []
    for name, leg in cs.gpu_legs().items():
        if leg.name == "h":
            for on in (True, False, True):
                recorded += cs.promised(leg, {"timing": on})
            recorded += [({"leg": "h", "timing": a}, {"leg": "h", "timing": b}) for a, b in ((True, False), (False, True))]
        else:
            recorded += cs.promised(leg)
    assert cs.missing_transitions(recorded) == []
    assert {r[2]["leg"] for r in cs.REQUIRED} == {leg.name for leg in cs.gpu_legs().values()}
    # a list that cannot be met is noticed: one leg left out
    assert cs.missing_transitions([r for r in recorded if r[1]["leg"] != "e"]) != []


def test_every_reference_is_computable_on_the_cpu(legs):
    for leg in legs.values():
        for s in leg.steps:
            assert s.ref is not None, (leg.name, s)


@pytest.mark.parametrize("name", list(cs.cpu_legs()))
def test_every_order_passes_on_a_kernel_set_without_state(legs, name):
    from helmholtz_kernels import HelmholtzOracleKernels
    leg = legs[name]
    K = HelmholtzOracleKernels()          # ONE for all orders of the leg
    recorded = []
    ran = set()
    for order in leg.orders:
        order = [i for i in order if leg.steps[i].cpu]
        cs.run_order(K, leg, order, recorded)
        ran |= set(order)
    assert ran == {i for i, s in enumerate(leg.steps) if s.cpu}
    if name in ("a1", "a2", "a3", "a4", "e"):          # every step of these legs runs here: the whole of their list is met
        assert cs.missing_transitions(recorded, legs={leg.name}) == []
