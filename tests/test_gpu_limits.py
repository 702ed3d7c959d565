"""The edges of the shape range on the device (tests/_limit_cases.py): what the emulation only has twins for -- the wave-level sums,
the LDS-DMA window prefetch, the bank and alignment behaviour at 5 .. 8 lanes per barcode, the generic-T instances' register budget."""
import pytest

import _limit_cases as c

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("name", sorted(c.STEP))
def test_step_at_the_edge_against_the_oracle_loop(hip_lib, monkeypatch, name, S):
    c.case_step(hip_lib, monkeypatch, name, S, "hip")


@pytest.mark.parametrize("name", sorted(c.RESIDENT))
def test_step_at_the_edge_resident_equals_two_kernel(hip_lib, monkeypatch, name):
    c.case_step_modes(hip_lib, monkeypatch, name, "hip")


@pytest.mark.parametrize("key", sorted(c.BOUNDARY), ids=lambda k: "-".join(map(str, k)))
def test_create_boundary_last_accepted_shape_works(hip_lib, key):
    c.case_boundary_accepted(hip_lib, key)


@pytest.mark.parametrize("key", sorted(c.BOUNDARY), ids=lambda k: "-".join(map(str, k)))
def test_create_boundary_first_refused_shape(hip_lib, key):
    c.case_boundary_refused(hip_lib, key)


@pytest.mark.parametrize("key", sorted(c.BOUNDARY), ids=lambda k: "-".join(map(str, k)))
def test_create_boundary_by_bisection(hip_lib, key):
    assert c.largest_T(hip_lib, *key) == c.BOUNDARY[key]


@pytest.fixture(scope="module")
def hier(hip_lib):
    """The handles of the HIER cases, each made once (three steps into a run) and shared by the tests below, which leave its
    parameters as they found them."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = c.HierHandle(hip_lib, name)
        return made[name]
    yield get
    for hh in made.values():
        hh.close()


@pytest.mark.parametrize("name,n", [(name, n) for name in sorted(c.HIER) for n in c.HIER_N[name]])
def test_hier_fitness_every_unit(hier, name, n):
    c.case_hier_all_units(hier(name), n)


@pytest.mark.parametrize("name", sorted(c.HIER))
def test_hier_fitness_refuses_sample_counts_outside_2_to_16384(hier, name):
    c.case_hier_bad_n(hier(name))


@pytest.mark.parametrize("name", sorted(c.HIER))
def test_hier_fitness_degenerate_posterior(hier, name):
    c.case_hier_degenerate(hier(name))
