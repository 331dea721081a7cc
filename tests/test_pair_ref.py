"""CPU checks of the paired dataset (training.PairedImageRestoration), its validation set (training.TestPairsCSV),
the numpy restatement of grr_patch_pair_batch (tests/pair_ref.py) and the restore command's --reference option."""
import importlib.util
import logging
import os

import numpy as np
import pytest

from irdu_amd import training
from tests import pair_ref, patch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    folder = tmp_path_factory.mktemp("pairs")
    csv_path, inputs, targets = pair_ref.write_pairs(str(folder))
    patch_ref.write_pictures(str(folder))          # the unpaired csv of the same sizes, for the plan
    return str(folder), csv_path, inputs, targets


def paired(pairs, name, **over):
    conf = dict(patch_ref.GOLDEN_CONFIGS[name])
    conf.update(over)
    return training.PairedImageRestoration(csv_path=pairs[1], root_folder=pairs[0], logger=logging.getLogger("test"),
                                           **conf)


@pytest.fixture(scope="module")
def command():
    spec = importlib.util.spec_from_file_location("restore_command", os.path.join(ROOT, "restore.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pair_ref_is_patch_ref_twice():
    """The restatement: target and input are patch_batch_ref's clean patch of either picture, the noise is
    patch_batch_ref's, and the pictures differ in every patch."""
    tgt, inp = [patch_ref.picture(0, 20, 24)], [patch_ref.picture(pair_ref.DEGRADED, 20, 24)]
    rows, ids, sigma = [(0, 3, 5, 3), (0, 19, 23, 1)], [11, (4 << 32) | 2], [0.1, 0.2]
    target, got, noise = pair_ref.pair_batch_ref(inp, tgt, rows, ids, sigma, 99, 16, 16)
    clean_t, _, noise_t = patch_ref.patch_batch_ref(tgt, rows, ids, sigma, 99, 16, 16)
    clean_i, noisy_i, _ = patch_ref.patch_batch_ref(inp, rows, ids, sigma, 99, 16, 16)
    assert np.array_equal(target, clean_t) and np.array_equal(got, noisy_i) and np.array_equal(noise, noise_t)
    target0, got0, noise0 = pair_ref.pair_batch_ref(inp, tgt, rows, ids, None, 99, 16, 16)
    assert np.array_equal(target0, clean_t) and np.array_equal(got0, clean_i) and not noise0.any()
    assert all((got0[s] != target0[s]).any() for s in range(2))


@pytest.mark.parametrize("name", sorted(patch_ref.GOLDEN_CONFIGS))
def test_dataset_selects_the_unpaired_plan(pairs, name):
    conf = dict(patch_ref.GOLDEN_CONFIGS[name])
    plain = training.ImageSuperResolution(csv_path=os.path.join(pairs[0], "info.csv"), root_folder=pairs[0],
                                          logger=logging.getLogger("test"), **conf)
    ds = paired(pairs, name)
    assert training.DATASETS["PairedImageRestoration"] is training.PairedImageRestoration
    assert len(ds) == len(plain) and ds.patchs_data == plain.patchs_data and np.array_equal(ds.plan, plain.plan)
    ds.random_permute(2024 + 2)
    plain.random_permute(2024 + 2)
    assert ds.epoch == 2 and np.array_equal(ds.plan, plain.plan)
    assert paired(pairs, name, dist_mode="none").patchs_data != [] and ds.dist_mode == conf["dist_mode"]


def test_getitem_none_is_the_two_files_at_one_crop_and_mode(pairs):
    _, _, inputs, targets = pairs
    ds = paired(pairs, "aug16", dist_mode="none", lambda_noise=None)
    rs = paired(pairs, "aug16", dist_mode="none", lambda_noise=None).random_state     # a twin of ds's stream
    seen = set()
    for i in range(12):
        row, col, _, img = ds.patchs_data[i]
        mode = rs.randint(0, 7)                # the parent's draw: the mode, and with "none" nothing else
        inp, tgt = ds[i]
        want_i = patch_ref.transform(patch_ref.clean_patch(inputs[img], row, col, 16, 16), mode)
        want_t = patch_ref.transform(patch_ref.clean_patch(targets[img], row, col, 16, 16), mode)
        assert inp.numpy().dtype == tgt.numpy().dtype == np.float32 and tuple(inp.shape) == (16, 16, 3)
        assert np.array_equal(inp.numpy(), want_i.astype(np.float32) / np.float32(255.0)), i
        assert np.array_equal(tgt.numpy(), want_t.astype(np.float32) / np.float32(255.0)), i
        assert (inp.numpy() != tgt.numpy()).any()
        seen.add(mode)
    assert len(seen) > 2
    # a patch larger than the picture: both are filled by the same mirror
    big = paired(pairs, "vary64", dist_mode="none", lambda_noise=None)
    k = next(i for i, r in enumerate(big.patchs_data) if r[3] == 0)
    inp, tgt = big[k]
    assert np.array_equal(inp.numpy(), patch_ref.clean_patch(inputs[0], 0, 0, 64, 64).astype(np.float32) / np.float32(255.0))
    assert np.array_equal(tgt.numpy(), patch_ref.clean_patch(targets[0], 0, 0, 64, 64).astype(np.float32) / np.float32(255.0))


def test_getitem_noise_modes_draw_as_the_parent_on_top_of_the_degraded_file(pairs):
    _, _, inputs, targets = pairs
    ds, twin = paired(pairs, "aug16"), paired(pairs, "aug16")
    rs = twin.random_state
    for i in range(3):
        row, col, _, img = ds.patchs_data[i]
        mode = rs.randint(0, 7)
        degraded = patch_ref.transform(patch_ref.clean_patch(inputs[img], row, col, 16, 16), mode).astype(np.float32) / 255.0
        want = training._noisy(degraded, rs, "addictive_noise_scale", 25.0)
        inp, tgt = ds[i]
        assert np.array_equal(inp.numpy(), want), i
        assert np.array_equal(tgt.numpy(), patch_ref.transform(
            patch_ref.clean_patch(targets[img], row, col, 16, 16), mode).astype(np.float32) / np.float32(255.0))


def test_value_errors(pairs, tmp_path):
    from PIL import Image
    with pytest.raises(ValueError, match="dist_mode"):
        paired(pairs, "aug16", dist_mode="jpeg")
    with pytest.raises(ValueError, match="dist_mode"):       # "none" is the paired dataset's alone
        training.ImageSuperResolution(csv_path=os.path.join(pairs[0], "info.csv"), root_folder=pairs[0],
                                      dist_mode="none", lambda_noise=None)
    csv_path, _, _ = pair_ref.write_pairs(str(tmp_path), shapes=((20, 24), (18, 30)))
    Image.fromarray(patch_ref.picture(1, 30, 18)).save(os.path.join(str(tmp_path), "clean1.png"))     # turned
    ds = training.PairedImageRestoration(csv_path=csv_path, root_folder=str(tmp_path), patch_size=16, max_num_patchs=4)
    assert ds.dist_mode == "none" and ds.load_image(0).shape == ds.load_target(0).shape == (20, 24, 3)
    with pytest.raises(ValueError, match=r"clean1\.png.*noisy1\.png"):
        ds.load_target(1)
    k = next(i for i, r in enumerate(ds.patchs_data) if r[3] == 1)
    with pytest.raises(ValueError, match=r"clean1\.png.*noisy1\.png"):
        ds[k]
    Image.fromarray(patch_ref.picture(1, 18, 30)[:, :, 0]).save(os.path.join(str(tmp_path), "clean1.png"))      # grey
    with pytest.raises(ValueError, match=r"clean1\.png.*noisy1\.png"):
        ds.load_target(1)
    other = tmp_path / "nocolumn"
    other.mkdir()
    bare, _, _ = pair_ref.write_pairs(str(other), shapes=((20, 24),), column=False)
    with pytest.raises(ValueError, match="target_path"):
        training.PairedImageRestoration(csv_path=bare, root_folder=str(other), patch_size=16)


def test_device_loader_draws_and_tables_without_a_gpu(pairs, monkeypatch):
    """The launch stubbed out: two arenas under one table, each file decoded once, both under one key of the
    shared dict; "none" draws the modes only and sends no sigma."""
    import torch
    from irdu_amd import kernels as K
    sent, decoded = [], []
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    monkeypatch.setattr(K, "_patch_pair_batch", lambda source, table, ids, sigma, *rest: sent.append(
        (table.numpy().copy(), ids.numpy().copy(), None if sigma is None else sigma.numpy().copy(), rest)) or (None, None))
    monkeypatch.setattr(training.DevicePatchLoader, "CHUNK_BYTES", 20000)
    load = training.PairedImageRestoration._load
    monkeypatch.setattr(training.PairedImageRestoration, "_load", lambda self, path: decoded.append(path) or load(self, path))
    ds = paired(pairs, "aug16", dist_mode="none", lambda_noise=None)
    shared, cpu = {}, torch.device("cpu")
    a = training.DevicePatchLoader(ds, training.ResumeableSampler(ds, 4), 4, device=cpu, shared=shared)
    inp, tgt = a.prepare()
    assert len(decoded) == 4 and len(shared) == 1 and inp.table is tgt.table and inp.host_table == tgt.host_table
    for i in range(4):
        assert np.array_equal(inp.image(i).numpy(), pairs[2][i]) and np.array_equal(tgt.image(i).numpy(), pairs[3][i])
    modes, sigma = a.epoch_draws(0)
    rs = np.random.RandomState((2204 * 1000003 + 0) % 2 ** 32)
    assert np.array_equal(modes, rs.randint(0, 8, len(ds))) and sigma.dtype == np.float32 and not sigma.any()
    assert len(list(a)) == 10
    rows = np.concatenate([s[0] for s in sent])
    assert np.array_equal(rows[:, :3], ds.plan) and np.array_equal(rows[:, 3], modes)
    assert all(s[2] is None for s in sent) and sent[0][3] == (2204, 16, 16)
    noisy = paired(pairs, "aug16", patch_size=32)
    b = training.DevicePatchLoader(noisy, training.ResumeableSampler(noisy, 4), 4, device=cpu, shared=shared)
    assert b.prepare()[0] is inp and b.prepare()[1] is tgt and len(shared) == 1 and len(decoded) == 4
    del sent[:]
    b.batch([0, 1])
    assert np.array_equal(sent[0][2], np.full(2, np.float32(25.0 / 255.0)))


def test_stage_accepts_device_resident_pairs(pairs):
    stage = lambda size: dict(type="PairedImageRestoration", device_resident=True, dataloader_args=dict(batch_size=2),
                              dataset_args=dict(csv_path=pairs[1], root_folder=pairs[0], patch_size=size,
                                                max_num_patchs=8))
    stages = training.build_train_stages(dict(datasets=dict(train=[stage(16), stage(32)])))
    assert all(isinstance(st.loader, training.DevicePatchLoader) and st.loader.paired for st in stages)
    assert stages[0].loader.shared is stages[1].loader.shared


def test_test_pairs_csv_yields_uint8_pairs(pairs, tmp_path):
    folder, _, inputs, targets = pairs
    csv_path = tmp_path / "val.csv"
    csv_path.write_text("index,path,target_path\n0,noisy0.png,clean0.png\n1,noisy2.png,clean2.png\n")
    assert training.VAL_DATASETS["TestPairsCSV"] is training.TestPairsCSV
    val, args = training.create_val_dataset(dict(datasets=dict(val=dict(
        type="TestPairsCSV", dataset_args=dict(csv_path=str(csv_path), root_folder=folder), factor=8, tile=64))))
    assert isinstance(val, training.TestPairsCSV) and args == dict(factor=8, tile=64) and len(val) == 2
    for k, i in enumerate((0, 2)):
        inp, tgt = val[k]
        assert inp.dtype == tgt.dtype == np.uint8
        assert np.array_equal(inp, inputs[i]) and np.array_equal(tgt, targets[i])
    bad = tmp_path / "bad.csv"
    bad.write_text("index,path\n0,noisy0.png\n")
    with pytest.raises(ValueError, match="target_path"):
        training.TestPairsCSV(str(bad), root_folder=folder)
    mixed = tmp_path / "mixed.csv"
    mixed.write_text("index,path,target_path\n0,noisy0.png,clean1.png\n")
    with pytest.raises(ValueError, match=r"noisy0\.png.*clean1\.png"):
        training.TestPairsCSV(str(mixed), root_folder=folder)[0]


def test_command_reference_option(command, pairs, tmp_path, capsys):
    base = ["-yaml_path", "conf.yaml", "--input", "in", "--output", "out"]
    args = command.parse_args(base + ["--reference", "refs", "--ssim", "--batch-images", "--self-ensemble"])
    assert args.reference == "refs" and args.sigma is None and args.ssim and args.batch_images and args.ensemble == 8
    assert command.parse_args(base + ["--reference", "refs", "--ensemble-modes", "0,1,4"]).ensemble == (0, 1, 4)
    assert command.parse_args(base + ["--sigma", "25"]).reference is None
    for bad in (["--reference", "refs", "--sigma", "25"], ["--ssim"]):
        with pytest.raises(SystemExit):
            command.parse_args(base + bad)
    capsys.readouterr()
    from PIL import Image
    ins, refs = tmp_path / "in", tmp_path / "refs"
    ins.mkdir()
    refs.mkdir()
    for k, (name, ref) in enumerate((("a.png", "a.bmp"), ("b.png", "b.png"))):
        Image.fromarray(patch_ref.picture(k + pair_ref.DEGRADED, 12, 14)).save(str(ins / name))
        Image.fromarray(patch_ref.picture(k, 12, 14)).save(str(refs / ref))
    (refs / "notes.txt").write_text("not an image")
    files = command.input_files(str(ins))
    found = command.reference_files(files, str(refs))
    assert [os.path.basename(f) for f in found] == ["a.bmp", "b.png"]
    command.check_references(files, found)
    Image.fromarray(patch_ref.picture(2, 12, 14)).save(str(ins / "c.png"))
    with pytest.raises(SystemExit, match=r"c\.png has no reference"):
        command.reference_files(command.input_files(str(ins)), str(refs))
    Image.fromarray(patch_ref.picture(2, 14, 12)).save(str(refs / "c.png"))
    files = command.input_files(str(ins))
    with pytest.raises(SystemExit, match=r"c\.png is 14x12x3.*c\.png is 12x14x3"):
        command.check_references(files, command.reference_files(files, str(refs)))
    Image.fromarray(patch_ref.picture(2, 12, 14)).save(str(refs / "c.jpg"))
    with pytest.raises(SystemExit, match=r"c\.png has 2 reference"):
        command.reference_files(files, str(refs))
    with pytest.raises(SystemExit, match="not a directory"):
        command.reference_files(files, str(tmp_path / "nowhere"))


def test_paired_example_yaml_names_registered_types():
    conf = training.parse(os.path.join(ROOT, "experiment_conf", "paired_example.yaml"))
    stages = training.train_stage_confs(conf)
    assert len(stages) == 2 and all(st["type"] == "PairedImageRestoration" and st["device_resident"] for st in stages)
    assert all(st["type"] in training.DATASETS for st in stages)
    assert len({st["dataset_args"]["csv_path"] for st in stages}) == 1          # one csv: the stages share the arenas
    assert conf["datasets"]["val"]["type"] == "TestPairsCSV" and conf["train"]["val_every"] > 0
