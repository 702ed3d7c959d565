"""The edges of the shape range in the host emulation (tests/_limit_cases.py): the step paths at the top of the resident range and
one past it, the create boundary, bb_hier_fitness on every unit and at the ends of n_samples."""
import pytest

import _limit_cases as c


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("name", sorted(c.STEP))
def test_step_at_the_edge_against_the_oracle_loop(emu_lib, monkeypatch, name, S):
    c.case_step(emu_lib, monkeypatch, name, S, "emu")


@pytest.mark.parametrize("name", sorted(c.RESIDENT))
def test_step_at_the_edge_resident_equals_two_kernel(emu_lib, monkeypatch, name):
    c.case_step_modes(emu_lib, monkeypatch, name, "emu")


def test_every_k_res_target_is_a_k_res_case():
    """The table's own shape: sections 1 - 4 name k_res, by both spellings; one past the edge nothing does."""
    for name, case in c.STEP.items():
        past = name in ("fitness_T17", "fitness_T18", "replicate_ragged_66") or name.endswith("_default")
        assert (name in c.K_RES) == (not past), name
        for S in (1, 2):
            n = case["names"][S]
            assert n["emu"].startswith("emu:") and not n["hip"].startswith("emu:") and "*" not in n["hip"], n
            assert (n["impl"]["emu"] == 2) == n["emu"].startswith("emu:k_res<"), n
            assert (n["impl"]["hip"] == 2) == n["hip"].startswith("k_res<"), n


@pytest.mark.parametrize("key", sorted(c.BOUNDARY), ids=lambda k: "-".join(map(str, k)))
def test_create_boundary_last_accepted_shape_works(emu_lib, key):
    c.case_boundary_accepted(emu_lib, key)


@pytest.mark.parametrize("key", sorted(c.BOUNDARY), ids=lambda k: "-".join(map(str, k)))
def test_create_boundary_first_refused_shape(emu_lib, key):
    c.case_boundary_refused(emu_lib, key)


@pytest.mark.parametrize("key", sorted(c.BOUNDARY), ids=lambda k: "-".join(map(str, k)))
def test_create_boundary_by_bisection(emu_lib, key):
    assert c.largest_T(emu_lib, *key) == c.BOUNDARY[key]


@pytest.fixture(scope="module")
def hier(emu_lib):
    """The handles of the HIER cases, each made once (three steps into a run) and shared by the tests below, which leave its
    parameters as they found them."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = c.HierHandle(emu_lib, name)
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
