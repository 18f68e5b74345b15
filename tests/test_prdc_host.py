"""CPU: the float64 restatement of precision / recall / density / coverage (tests/prdc_ref.py) against the reference's own
numbers -- tests/golden/pr.npz and tests/golden/group_eval.npz (tools/gen_goldens_group_eval.py) -- and, where the reference has
no counterpart (density, coverage), against double loops and the metrics' defining properties.

The reference computes in fp32, the restatement in float64: a fraction may differ by the samples that have a comparison within
fp32 rounding of its radius (prdc_ref.borderline), and by no more."""
import os

import numpy as np
import pytest

import prdc_ref as R


@pytest.fixture(scope="module")
def pr(golden_dir):
    return np.load(os.path.join(golden_dir, "pr.npz"))


@pytest.fixture(scope="module")
def ge(golden_dir):
    return np.load(os.path.join(golden_dir, "group_eval.npz"))


def _check_pr(ref_precision, ref_recall, real, fake, k):
    got = R.prdc(real, fake, k)
    slack_r = R.borderline(got['D'], got['fake_radii'][None, :]).any(axis=1).sum()
    slack_p = R.borderline(got['D'], got['real_radii'][:, None]).any(axis=0).sum()
    print(f"\nprecision {got['precision']:.6f} (reference {ref_precision:.6f}, {slack_p} borderline), "
          f"recall {got['recall']:.6f} (reference {ref_recall:.6f}, {slack_r} borderline)")
    assert abs(got['precision'] - ref_precision) <= slack_p / fake.shape[0] + 1e-12
    assert abs(got['recall'] - ref_recall) <= slack_r / real.shape[0] + 1e-12
    return got


def test_restatement_matches_the_reference_on_pr_npz(pr):
    k = int(pr["nearest_k"])
    got = _check_pr(float(pr["precision"]), float(pr["recall"]), pr["real"], pr["fake"], k)
    np.testing.assert_allclose(got['real_radii'], pr["radii"], rtol=2e-5, atol=2e-4)
    np.testing.assert_allclose(got['D'][:64, :48], pr["dist"], rtol=2e-5, atol=2e-4)
    slack = R.borderline(got['D'][:100], got['fake_radii'][None, :]).any(axis=1).sum()
    assert abs(R.partial_recall(pr["real"][:100], pr["fake"], k) - float(pr["partial_recall"])) <= slack / 100 + 1e-12
    assert R.partial_recall(pr["real"][:100], pr["fake"], k) == got['real_hit'][:100].mean()


def test_restatement_matches_the_reference_on_the_probe_set(ge):
    real, fake = R.probe_set(0)
    np.testing.assert_array_equal(real, ge["real"])
    np.testing.assert_array_equal(fake, ge["fake"])
    assert int(ge["nearest_k"]) == R.PROBE_K
    got = _check_pr(float(ge["precision"]), float(ge["recall"]), real, fake, R.PROBE_K)
    edge = R.borderline(got['D'], got['fake_radii'][None, :]).any(axis=1)
    for name, idx in R.probe_groups().items():
        np.testing.assert_array_equal(idx, ge[f"index_{name}"])
        mine = R.partial_recall(real[idx], fake, R.PROBE_K)
        assert mine == got['real_hit'][idx].mean()                  # a group's recall reduces from the whole set's flags
        assert abs(mine - float(ge[f"partial_recall_{name}"])) <= edge[idx].sum() / len(idx) + 1e-12, name
    groups = R.probe_groups()
    assert len(groups['g40']) == 40 and len(np.intersect1d(groups['low'], groups['odd'])) > 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_density_and_coverage_against_double_loops(seed):
    rng = np.random.default_rng(seed)
    real = rng.normal(size=(23, 5))
    fake = rng.normal(size=(31, 5)) * 1.2 + 0.2
    got, loops = R.prdc(real, fake, 3), R.prdc_loops(real, fake, 3)
    for key in ('precision', 'recall', 'density', 'coverage'):
        assert got[key] == loops[key], key
    assert 0 < got['coverage'] <= 1 and got['density'] > 0
    assert got['fake_count'].sum() == (got['D'] < got['real_radii'][:, None]).sum()
    np.testing.assert_array_equal(got['fake_hit'], got['fake_count'] > 0)


def test_identical_and_far_apart_sets():
    rng = np.random.default_rng(3)
    a = rng.normal(size=(60, 8))
    same = R.prdc(a, a.copy(), 3)
    assert same['coverage'] == 1.0 and same['precision'] == 1.0 and same['recall'] == 1.0
    assert same['density'] >= 1.0                  # every ball holds its centre and the k - 1 neighbours strictly inside it
    far = R.prdc(a, a + 100.0, 3)
    assert [far[k] for k in ('precision', 'recall', 'density', 'coverage')] == [0.0, 0.0, 0.0, 0.0]
