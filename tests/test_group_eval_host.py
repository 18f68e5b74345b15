"""CPU: the host side of evaluation by group -- the attribute file's parsing against the reference's own results
(tests/golden/group_eval.npz), the flag tables of the five scripts against the reference's names and defaults, output file names,
the argument checks' messages, and the group means of disc_score_celeba_with_attr."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def ge(golden_dir):
    return np.load(os.path.join(golden_dir, "group_eval.npz"))


@pytest.fixture()
def attr_root(ge, tmp_path):
    os.makedirs(tmp_path / "celeba")
    (tmp_path / "celeba" / "list_attr_celeba.txt").write_bytes(ge["attr_text"].tobytes())
    return str(tmp_path)


def test_attribute_indices_are_the_reference_s(ge, attr_root):
    from diagan.datasets.get_celeba_index_with_attr import get_celeba_index_with_attr, read_attr_table, restrict
    names, values = read_attr_table(attr_root)
    assert names == list(ge["attr_names"]) and values.shape == (12, len(names)) and set(np.unique(values)) <= {0, 1}
    for name in names:
        a, b = get_celeba_index_with_attr(attr_root, name)
        assert isinstance(a, list) and isinstance(b, list)
        np.testing.assert_array_equal(a, ge[f"attr_index_{name}"])
        np.testing.assert_array_equal(b, ge[f"not_attr_index_{name}"])
        assert sorted(a + b) == list(range(12))
    with pytest.raises(ValueError) as e:
        get_celeba_index_with_attr(attr_root, "No_Such_Attribute")
    assert str(e.value) == str(ge["invalid_message"]) == "Invalid attribute name No_Such_Attribute."
    np.testing.assert_array_equal(restrict([0, 3, 11, 7, 8], 8), [0, 3, 7])


def test_groups_are_cut_after_seeding_attribute_first(ge, attr_root):
    """The reference's draw (image_loader_with_attr.py:35-43): np.random.choice without replacement, with-attribute first."""
    from diagan.trainer import group_eval as G
    assert G.attr_names(attr_root, "Bald") == ["Bald"] and G.attr_names(attr_root, "Male,Young") == ["Male", "Young"]
    assert G.attr_names(attr_root, "all") == list(ge["attr_names"])
    np.random.seed(4)
    got = G.attr_groups(attr_root, ["Smiling", "Bald"], num_rows=10, num_samples=3, verbose=False)
    np.random.seed(4)
    want = {}
    for name in ("Smiling", "Bald"):
        a, b = (ge[f"{side}_{name}"][ge[f"{side}_{name}"] < 10] for side in ("attr_index", "not_attr_index"))
        a = np.random.choice(a, size=3, replace=False) if len(a) > 3 else a
        b = np.random.choice(b, size=3, replace=False) if len(b) > 3 else b
        want[name] = (a, b)
    assert list(got) == ["Smiling", "Bald"]
    for name in want:
        np.testing.assert_array_equal(got[name][0], want[name][0])
        np.testing.assert_array_equal(got[name][1], want[name][1])
    assert len(got["Bald"][0]) == 2 and len(got["Bald"][1]) == 3           # rows 2 and 9 are bald: nothing to cut
    with pytest.raises(ValueError, match="Invalid attribute name Hat."):
        G.attr_groups(attr_root, ["Hat"], 10)


# flag -> default of the reference's scripts (eval_gan_with_index.py:25-42, eval_gan_celeba_with_attr.py:15-29,
# disc_score_celeba_with_attr.py:12-20); --gpu is '0' there and unset here, as in eval_gan.py
REF_INDEX = {"--dataset": "cifar10", "--work_dir": "./exp_results", "--exp_name": "mimicry_pretrained-seed1",
             "--baseline_exp_name": None, "--p1_step": 40000, "--model": "sngan", "--loss_type": "hinge", "--gpu": None,
             "--batch_size": 128, "--seed": 1, "--netG_ckpt_step": None, "--netG_train_mode": False, "--resample_score": None,
             "--gold": False, "--topk": False, "--index_num": 100}
REF_ATTR = {"--dataset": "celeba", "--root": "./dataset/celeba", "--attr": "Bald", "--work_dir": "./exp_results",
            "--exp_name": "mimicry_pretrained-seed1", "--model": "sngan", "--loss_type": "hinge", "--gpu": None,
            "--batch_size": 128, "--seed": 1, "--netG_ckpt_step": None, "--netG_train_mode": False}
REF_DISC = {"--dataset": "celeba", "--root": "./dataset/celeba", "--attr": "Bald", "--work_dir": "./exp_results",
            "--exp_name": "mimicry_pretrained-seed1", "--p1_step": 60000, "--resample_score": None}
SCRIPTS = [("eval_gan_with_index", REF_INDEX, False), ("eval_gan_drs_with_index", REF_INDEX, True),
           ("eval_gan_celeba_with_attr", REF_ATTR, False), ("eval_gan_drs_celeba_with_attr", REF_ATTR, True),
           ("disc_score_celeba_with_attr", REF_DISC, False)]


@pytest.mark.parametrize("script,ref,drs", SCRIPTS)
def test_cli_flag_surface(script, ref, drs):
    sys.path.insert(0, ROOT)
    mod = __import__(script)
    parser = mod.build_parser()
    opts = {s for a in parser._actions for s in a.option_strings}
    got = vars(parser.parse_args([]))
    ref = dict(ref, **({"--use_original_netD": False} if drs else {}))
    for flag, default in ref.items():
        assert flag in opts, flag
        assert got[flag[2:]] == default, flag
    assert ("--use_original_netD" in opts) == drs
    if "--dataset" in ref:
        assert "-d" in opts
    assert callable(mod.main)


@pytest.mark.parametrize("script", [s for s, _, _ in SCRIPTS])
def test_cli_help(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script + ".py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-800:]
    assert "--attr" in r.stdout or "--index_num" in r.stdout


def test_output_names_and_argument_checks(tmp_path):
    from diagan.trainer import evaluate as ev
    index = np.arange(100)
    kw = dict(name='high_ldr', num_fake_samples=50000)
    assert ev._index_output_name('fid', index, False, kw) == 'fid_high_ldr_100_50k.json'
    assert ev._index_output_name('fid', index, True, kw) == 'fid_high_ldr_drs_100_50k.json'
    pr = dict(num_real_samples=10000, num_fake_samples=10000)
    assert ev._attr_output_name('partial_recall', 'Bald', pr) == 'partial_recall_Bald_10k_10k.json'
    assert ev._attr_output_name('partial_prdc', 'Bald', pr) == 'partial_prdc_Bald_10k_10k.json'
    assert ev._attr_output_name('fid', 'Bald', pr) == 'fid_Bald_10k.json'
    assert ev.ATTR_METRICS == ['partial_recall', 'partial_prdc', 'fid']
    log = tmp_path / 'run'
    for fn, extra in ((ev.evaluate_with_index, dict(index=index)), (ev.evaluate_drs_with_index, dict(index=index, netD_drs=None)),
                      (ev.evaluate_with_attr, dict(attr='Bald')), (ev.evaluate_drs_with_attr, dict(attr='Bald', netD_drs=None))):
        metric = 'fid' if 'index' in extra else 'partial_recall'
        with pytest.raises(ValueError, match="Only one of evaluate_step or evaluate_range can be defined."):
            fn(metric, netG=None, log_dir=log, **extra)
        with pytest.raises(ValueError, match="Only one of evaluate_step or evaluate_range can be defined."):
            fn(metric, netG=None, log_dir=log, evaluate_step=5, evaluate_range=(1, 2, 1), **extra)
        with pytest.raises(ValueError, match=r"evaluate_range must be a tuple of ints \(start, end, step\)."):
            fn(metric, netG=None, log_dir=log, evaluate_range=[1, 2, 1], **extra)
        with pytest.raises(ValueError, match="Invalid metric kid selected. Choose from"):
            fn('kid', netG=None, log_dir=log, evaluate_step=5, **extra)
    with pytest.raises(ValueError, match="name and num_fake_samples must be provided for FID computation."):
        ev.evaluate_with_index('fid', index, None, log, evaluate_step=5, num_fake_samples=100)
    with pytest.raises(ValueError, match="num_real_samples and num_fake_samples must be provided for PR computation."):
        ev.evaluate_with_attr('partial_recall', 'Bald', None, log, evaluate_step=5, num_fake_samples=100)
    with pytest.raises(ValueError, match="Checkpoint directory .* cannot be found in log_dir."):
        ev.evaluate_with_index('fid', index, None, log, evaluate_step=5, **kw)
    assert not (log / 'evaluate' / 'step-5' / 'fid_high_ldr_100_50k.json').exists()


def test_disc_score_group_means_and_high_low_index(ge):
    from diagan import eval_cli
    w = np.random.default_rng(9).random(12)
    a, b = ge["attr_index_Bald"], ge["not_attr_index_Bald"]
    got = eval_cli.attr_weight_means(w, a, b)
    assert got == (w[[2, 9]].mean(), np.delete(w, [2, 9]).mean())
    cut = eval_cli.attr_weight_means(w, a, b, train_num=8)               # the reference keeps the rows below train_num
    assert cut == (w[[2]].mean(), np.delete(w[:8], [2]).mean())
    assert eval_cli.CELEBA_TRAIN_NUM == 162770
    high, low = eval_cli.high_low_index(w, 3)
    order = np.argsort(w)
    np.testing.assert_array_equal(high, order[-3:])
    np.testing.assert_array_equal(low, order[:3])
    assert w[high].min() > w[low].max()


def test_abi_header_of_its_own():
    """The PRDC entry points are declared in include/diagan_prdc.h and nowhere in diagan_hip.h; the library exports them."""
    import ctypes
    from diagan import _native as nat
    from diagan._native import prdc_abi as pnat
    sigs = pnat.signatures()
    assert set(sigs) == {"diagan_prdc_reduce", "diagan_prdc_reduce_ws"} and not set(sigs) & set(nat.signatures())
    assert sigs["diagan_prdc_reduce_ws"] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
    assert len(sigs["diagan_prdc_reduce"][1]) == 15
    L = ctypes.CDLL(nat.LIB_PATH)
    assert all(hasattr(L, n) for n in sigs)
    ws = pnat.fn("diagan_prdc_reduce_ws")
    assert ws(333, 517) == (2 * 1 * 333 + 6 * 517) * 4 and ws(0, 4) == 0 and ws(4, 0) == 0
    assert ws(8192, 10000) == (2 * 10 * 8192 + 128 * 10000) * 4
