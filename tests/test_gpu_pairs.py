"""grr_patch_pair_batch, the paired DevicePatchLoader, restore.evaluate_pairs and training on degraded / clean
pairs on the GPU, against the numpy restatement tests/pair_ref.py.

The arenas and patches are tests/test_gpu_patches.py's: pictures of 5 x 7, 16 x 16, 40 x 56 and 70 x 33 packed back
to back (images start at odd bytes), C = 1 and 3; patches of 16 x 16, 48 x 48 (several mirror periods, an odd turn
wider than one tile), 16 x 32 (even-k modes only) and 6 x 6 (the scalar stores).  The input picture k is
patch_ref.picture(k + 3 + 17), the target picture(k + 3), so swapping the two is visible in every sample."""
import logging
import os

import numpy as np
import pytest
import torch

from tests import pair_ref, patch_ref, ssim_ref
from tests.test_gpu_patches import PATCHES, SEED, SHAPES, rows_of

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
N = 37
DEV = "cuda:0"


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels, restore, training
    return type("G", (), dict(K=kernels, R=restore, T=training, I=irdu_amd))


def pictures_of(c):
    targets = [patch_ref.picture(k + 3, h, w, c) for k, (h, w) in enumerate(SHAPES)]
    inputs = [patch_ref.picture(k + 3 + pair_ref.DEGRADED, h, w, c) for k, (h, w) in enumerate(SHAPES)]
    return inputs, targets


_CASES = {}


def case(G, c, ph, pw):
    """The kernel's batches (without and with sigma) and the restatement's of one (C, patch) case, computed once."""
    key = (c, ph, pw)
    if key not in _CASES:
        inputs, targets = pictures_of(c)
        source = G.K.patch_pair_source(G.R.pack_images(inputs, DEV), G.R.pack_images(targets, DEV))
        rows = rows_of(N, ph, pw)
        ids = np.array([(3 << 32) | (s * 11 + 1) for s in range(N)], dtype=np.int64)
        sigma = np.array([(5.0, 25.0, 50.0)[s % 3] / 255.0 for s in range(N)], dtype=np.float32)
        plain = [t.cpu().numpy() for t in G.K.patch_pair_batch(source, rows, ids, None, SEED, ph, pw)]
        noised = [t.cpu().numpy() for t in G.K.patch_pair_batch(source, rows, ids, sigma, SEED, ph, pw)]
        ref_plain = pair_ref.pair_batch_ref(inputs, targets, rows, ids, None, SEED, ph, pw)
        ref_noised = pair_ref.pair_batch_ref(inputs, targets, rows, ids, sigma, SEED, ph, pw)
        for v in ref_plain + ref_noised:
            v.setflags(write=False)
        _CASES[key] = dict(inputs=inputs, targets=targets, source=source, rows=rows, ids=ids, sigma=sigma, plain=plain,
                           noised=noised, ref_plain=ref_plain, ref_noised=ref_noised)
    return _CASES[key]


@pytest.mark.parametrize("c", (1, 3))
@pytest.mark.parametrize("ph,pw", PATCHES)
def test_without_sigma_both_outputs_are_the_restatement_bit_for_bit(G, c, ph, pw):
    k = case(G, c, ph, pw)
    target, inp = k["plain"]
    assert target.shape == inp.shape == (N, c, ph, pw) and target.dtype == inp.dtype == np.float32
    assert np.array_equal(target, k["ref_plain"][0]) and np.array_equal(inp, k["ref_plain"][1])
    assert all((inp[s] != target[s]).any() for s in range(N))
    if ph == pw:
        assert {r[3] for r in k["rows"]} == set(range(8))
    # a zero sigma is no sigma
    t0, i0 = G.K.patch_pair_batch(k["source"], k["rows"], k["ids"], np.zeros(N, np.float32), SEED, ph, pw)
    assert np.array_equal(t0.cpu().numpy().view(np.int32), target.view(np.int32))
    assert np.array_equal(i0.cpu().numpy().view(np.int32), inp.view(np.int32))


@pytest.mark.parametrize("c,ph,pw", [(3, 48, 48), (1, 6, 6)])
def test_one_arena_twice_is_patch_batch(G, c, ph, pw):
    k = case(G, c, ph, pw)
    pack = k["source"].target
    clean, noisy = G.K.patch_batch(pack, k["rows"], k["ids"], k["sigma"], SEED, ph, pw)
    target, inp = G.K.patch_pair_batch(G.K.patch_pair_source(pack, pack), k["rows"], k["ids"], k["sigma"], SEED, ph, pw)
    assert torch.equal(target.view(torch.int32), clean.view(torch.int32))
    assert torch.equal(inp.view(torch.int32), noisy.view(torch.int32))
    assert not torch.equal(inp, target)


@pytest.mark.parametrize("c", (1, 3))
@pytest.mark.parametrize("ph,pw", PATCHES)
def test_with_sigma_the_input_is_within_the_noise_bound(G, c, ph, pw):
    """|input - ref| <= 2^-23 (|noise_ref| + |input_ref|), test_noisy_on_a_real_arena's bound: one ulp of the noise
    plus one of the sum.  The target is untouched."""
    k = case(G, c, ph, pw)
    target, inp = k["noised"]
    target_ref, inp_ref, noise_ref = k["ref_noised"]
    assert np.array_equal(target, target_ref) and np.array_equal(target, k["plain"][0])
    err = np.abs(inp.astype(np.float64) - inp_ref.astype(np.float64))
    bound = EPS * (np.abs(noise_ref).astype(np.float64) + np.abs(inp_ref).astype(np.float64))
    print(f"C {c} {ph}x{pw}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, "
          f"differing {np.count_nonzero(err)} of {err.size}")
    assert np.isfinite(inp).all() and (err <= bound).all()
    assert all((inp[s] != k["plain"][1][s]).any() for s in range(N))


@pytest.mark.parametrize("c,ph,pw", [(3, 48, 48), (1, 16, 32), (3, 6, 6)])
def test_a_sample_does_not_depend_on_its_batch(G, c, ph, pw):
    k = case(G, c, ph, pw)
    run = lambda idx, sigma=k["sigma"]: [t.cpu().numpy() for t in G.K.patch_pair_batch(
        k["source"], [k["rows"][i] for i in idx], k["ids"][idx], None if sigma is None else sigma[idx], SEED, ph, pw)]
    order = list(np.random.RandomState(1).permutation(N))
    for want, sigma in ((k["noised"], k["sigma"]), (k["plain"], None)):
        at = 0
        for size in (1, 5, 13, 18):                     # the shuffled rows in batches of other sizes
            idx = order[at:at + size]
            got = run(idx, sigma)
            assert np.array_equal(got[0], want[0][idx]) and np.array_equal(got[1], want[1][idx]), size
            at += size
        assert at == N


# ---------------------------------------------------------------------------
# the loader
@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    folder = tmp_path_factory.mktemp("pairs")
    csv_path, inputs, targets = pair_ref.write_pairs(str(folder))
    return str(folder), csv_path, inputs, targets


def loader_of(G, pairs, name="aug16", batch=4, rank=0, world=1, shared=None, **over):
    conf = dict(patch_ref.GOLDEN_CONFIGS[name])
    conf.update(over)
    ds = G.T.PairedImageRestoration(csv_path=pairs[1], root_folder=pairs[0], logger=logging.getLogger("test"), **conf)
    sampler = G.T.ResumeableSampler(ds, batch, rank, world)
    return G.T.DevicePatchLoader(ds, sampler, batch, device=torch.device(DEV), shared=shared)


def batches(loader):
    return [(i.cpu().numpy(), t.cpu().numpy()) for i, t in loader]


@pytest.mark.parametrize("name,over", [("aug16", dict(dist_mode="none", lambda_noise=None)), ("aug16", {}), ("vary64", {})])
def test_loader_batches_are_the_restatement_on_the_plan(G, pairs, name, over):
    loader = loader_of(G, pairs, name, **over)
    ds = loader.dataset
    loader.sampler.set_epoch_and_current_sample(2, -1)
    got = batches(loader)
    assert len(got) == len(loader) and all(i.shape == t.shape for i, t in got)
    modes, sigma = loader.epoch_draws(2)
    rows = [(img, r, c, modes[p]) for p, (r, c, _, img) in enumerate(ds.patchs_data)]
    ids = (2 << 32) | np.arange(len(ds), dtype=np.int64)
    ph, pw = ds.out_size()
    none = ds.dist_mode == "none"
    target_ref, inp_ref, noise_ref = pair_ref.pair_batch_ref(pairs[2], pairs[3], rows, ids, None if none else sigma,
                                                             ds.seed, ph, pw)
    inp, target = np.concatenate([i for i, _ in got]), np.concatenate([t for _, t in got])
    assert np.array_equal(target, target_ref)
    if none:
        assert np.array_equal(inp, inp_ref) and not sigma.any() and set(modes.tolist()) == set(range(8))
    else:
        assert (np.abs(inp.astype(np.float64) - inp_ref) <= EPS * (np.abs(noise_ref).astype(np.float64) + np.abs(inp_ref))).all()
        assert noise_ref.any()


def test_loader_resumes_bitwise(G, pairs):
    loader = loader_of(G, pairs)
    loader.sampler.set_epoch_and_current_sample(1, -1)
    full = batches(loader)
    assert len(full) == 10
    fresh = loader_of(G, pairs)                                  # another process's resume
    fresh.sampler.set_epoch_and_current_sample(1, 3 * 4 - 1)
    rest = batches(fresh)
    assert len(rest) == 7
    for (i0, t0), (i1, t1) in zip(full[3:], rest):
        assert np.array_equal(i0, i1) and np.array_equal(t0, t1)
    loader.sampler.set_epoch_and_current_sample(2, -1)
    assert not any(np.array_equal(a[0], b[0]) for a, b in zip(full, batches(loader)))


def test_two_ranks_make_the_one_rank_global_batch(G, pairs):
    one = loader_of(G, pairs, batch=8)
    ranks = [loader_of(G, pairs, batch=4, rank=r, world=2) for r in (0, 1)]
    for ld in [one] + ranks:
        ld.sampler.set_epoch_and_current_sample(0, -1)
    whole, parts = batches(one), [batches(ld) for ld in ranks]
    assert len(whole) == len(parts[0]) == len(parts[1]) == 5
    for gb, p0, p1 in zip(whole, *parts):
        assert np.array_equal(gb[0], np.concatenate([p0[0], p1[0]]))
        assert np.array_equal(gb[1], np.concatenate([p0[1], p1[1]]))


def test_two_stages_over_one_csv_hold_the_same_two_arenas(G, pairs):
    shared = {}
    a = loader_of(G, pairs, shared=shared)
    b = loader_of(G, pairs, "vary64", shared=shared)
    (ia, ta), (ib, tb) = a.prepare(), b.prepare()
    assert ia.arena is ib.arena and ta.arena is tb.arena and ia.arena is not ta.arena and len(shared) == 1
    assert ia.arena.data_ptr() != ta.arena.data_ptr() and ia.table is ta.table
    for i in range(4):
        assert np.array_equal(ia.image(i).cpu().numpy(), pairs[2][i])
        assert np.array_equal(ta.image(i).cpu().numpy(), pairs[3][i])
    assert loader_of(G, pairs).prepare()[0].arena is not ia.arena            # no dict, no sharing


# ---------------------------------------------------------------------------
# evaluation
EVAL_SIZES = [(40, 56), (37, 53), (100, 140), (64, 64)]      # 37 x 53: no multiple of 16; 100 x 140: larger than tile
TILING = dict(factor=16, tile=64, halo=16, device=DEV)


def eval_pairs(c=3):
    targets = [patch_ref.picture(k, h, w, c) for k, (h, w) in enumerate(EVAL_SIZES)]
    # a degraded version that is close to its target, so the PSNR is a plausible one
    rs = np.random.RandomState(4)
    inputs = [np.clip(t.astype(np.int64) + rs.randint(-9, 10, t.shape), 0, 255).astype(np.uint8) for t in targets]
    return inputs, targets


def identity(x):
    return x


def blur(x):
    """A fixed 3 x 3 box blur: batch-independent, any window size."""
    return torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), 3, 1)


def test_evaluate_pairs_of_the_identity_is_the_host_psnr_and_the_restatement_ssim(G):
    inputs, targets = eval_pairs()
    got = G.R.evaluate_pairs(identity, inputs, targets, metrics=("psnr", "ssim"), **TILING)
    assert set(got) == {"psnr", "ssim"}
    for a, b, psnr, ssim in zip(inputs, targets, got["psnr"][1], got["ssim"][1]):
        sse = int(np.sum((a.astype(np.int64) - b.astype(np.int64)) ** 2, dtype=np.int64))
        assert sse > 0 and psnr == float(10.0 * np.log10(255.0 ** 2 * a.size / sse))
        assert abs(ssim - ssim_ref.ssim(a, b)) <= 2.0 ** -32
    for m in ("psnr", "ssim"):
        assert got[m][0] == float(np.mean(got[m][1])) and len(got[m][1]) == len(inputs)
    assert G.R.evaluate_pairs(identity, inputs, targets, **TILING) == {"psnr": got["psnr"]}
    assert G.R.evaluate_pairs(identity, targets, targets, **TILING)["psnr"][0] == float("inf")
    # tensors, on the host and on the device, are taken as they are
    mixed = [torch.from_numpy(inputs[0]), torch.from_numpy(inputs[1]).to(DEV)] + inputs[2:]
    assert G.R.evaluate_pairs(identity, mixed, targets, metrics=("psnr", "ssim"), **TILING) == got


@pytest.mark.parametrize("model", [identity, blur])
@pytest.mark.parametrize("ensemble", [1, (0, 1)])
def test_evaluate_pairs_per_image_and_across_images_are_equal(G, model, ensemble):
    inputs, targets = eval_pairs()
    args = dict(metrics=("psnr", "ssim"), ensemble=ensemble, **TILING)
    per = G.R.evaluate_pairs(model, inputs, targets, **args)
    assert per == G.R.evaluate_pairs(model, inputs, targets, across_images=True, **args)
    for a, b, psnr, ssim in zip(inputs, targets, per["psnr"][1], per["ssim"][1]):
        restored = G.R.restore_image(model, a, ensemble=ensemble, **TILING)
        assert restored.dtype == np.uint8 and psnr == G.R.psnr_u8(restored, b) and ssim == G.R.ssim_u8(restored, b)


def test_evaluate_pairs_of_a_seeded_model_is_restore_image_then_psnr(G):
    inputs, targets = eval_pairs()
    torch.manual_seed(5)
    model = G.I.GLRImageFilter(n_channels_in=3, n_channels_out=3, ngraphs=4, n_cgd_iters=1).to(DEV)
    mean, values = G.R.evaluate_pairs(model, inputs, targets, factor=16, tile=64, halo=16)["psnr"]
    want = [G.R.psnr_u8(G.R.restore_image(model, a, factor=16, tile=64, halo=16), b) for a, b in zip(inputs, targets)]
    assert values == want and mean == float(np.mean(want)) and all(np.isfinite(v) for v in values)
    assert values != G.R.evaluate_pairs(identity, inputs, targets, **TILING)["psnr"][1]


def test_evaluate_pairs_refuses_before_any_launch(G, monkeypatch):
    inputs, targets = eval_pairs()

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(G.K, "_launch", no_launch)
    with pytest.raises(ValueError, match="one target per input"):
        G.R.evaluate_pairs(identity, inputs, targets[:3], **TILING)
    with pytest.raises(ValueError, match="input 1 .*one shape"):
        G.R.evaluate_pairs(identity, inputs, [targets[0], targets[1][:, :50]] + targets[2:], **TILING)
    with pytest.raises(ValueError, match="target 2 .*uint8"):
        G.R.evaluate_pairs(identity, inputs, targets[:2] + [targets[2].astype(np.float32)] + targets[3:], **TILING)
    small = patch_ref.picture(0, 10, 40)
    with pytest.raises(ValueError, match="pair 4 .*SSIM"):
        G.R.evaluate_pairs(identity, inputs + [small], targets + [small], metrics=("ssim",), **TILING)
    with pytest.raises(ValueError, match="metrics"):
        G.R.evaluate_pairs(identity, inputs, targets, metrics=("mse",), **TILING)


# ---------------------------------------------------------------------------
# training
def paired_conf(pairs, root, total):
    folder, csv_path = pairs[0], pairs[1]
    val_csv = os.path.join(root, "val.csv")
    with open(val_csv, "w") as f:
        f.write("index,path,target_path\n0,noisy0.png,clean0.png\n1,noisy1.png,clean1.png\n")
    stage = lambda size, batch, **extra: dict(
        name=f"Training-pairs-{size}", type="PairedImageRestoration", device_resident=True,
        dataset_args=dict(csv_path=csv_path, root_folder=folder, use_data_aug=True, patch_size=[size, size],
                          max_num_patchs=8, **extra),
        dataloader_args=dict(batch_size=batch, num_workers=4))
    return dict(name="paired", manual_seed=2204, path=dict(root_dir=root),
                datasets=dict(train=[stage(16, 4), stage(32, 2, seed=2224, dist_mode="addictive_noise", lambda_noise=5.0)],
                              val=dict(type="TestPairsCSV", dataset_args=dict(csv_path=val_csv, root_folder=folder),
                                       factor=16, tile=64, halo=16)),
                model=dict(type="GLRImageFilter", args=dict(n_channels_in=3, n_channels_out=3, ngraphs=4, n_cgd_iters=1)),
                # no draw of torch's generator in the loss: a step is a function of the weights and the batch
                train=dict(total_iters=total, checkpoint_every=2, verbose_every=1, val_every=2, loss02_weight=0.0,
                           loss03_weight=0.0))


def test_run_trains_validates_checkpoints_and_resumes_bitwise(G, pairs, tmp_path):
    roots = [str(tmp_path / name) for name in ("whole", "resumed")]
    for root in roots:
        os.makedirs(root)
    dev = torch.device(DEV)
    torch.manual_seed(7)
    conf = paired_conf(pairs, roots[0], 4)
    whole = G.T.run(conf, device=dev)
    assert whole.i == 4 and len(whole.train_history) == 4
    assert all(np.isfinite(v) for row in whole.train_history for v in row)
    assert [i for i, _ in whole.val_history] == [2, 4]
    # the recorded values are validate_pairs': the model's PSNR on the two validation pairs, nothing drawn
    val = G.T.TestPairsCSV(**conf["datasets"]["val"]["dataset_args"])
    assert whole.val_history[-1][1] == G.T.validate_pairs(whole.model, val, factor=16, device=dev, tile=64, halo=16)
    want = G.R.evaluate_pairs(whole.model, [val[0][0], val[1][0]], [val[0][1], val[1][1]], factor=16, tile=64, halo=16)
    assert whole.val_history[-1][1] == want["psnr"][0] and np.isfinite(want["psnr"][0])
    assert sorted(os.listdir(G.T.checkpoint_dir(conf))) == ["checkpoint_iter00000002.pt", "checkpoint_iter00000004.pt"]

    torch.manual_seed(7)
    G.T.run(paired_conf(pairs, roots[1], 2), device=dev)
    resumed = G.T.run(paired_conf(pairs, roots[1], 4), device=dev)
    assert resumed.i == 4 and [i for i, _ in resumed.val_history] == [4]
    assert resumed.val_history[-1] == whole.val_history[-1]
    saved = [torch.load(os.path.join(root, "experiments", "paired", "learning_checkpoints", "checkpoint_iter00000004.pt"),
                        weights_only=True) for root in roots]
    assert saved[0]["i"] == saved[1]["i"] == 4 and set(saved[0]["model"]) == set(saved[1]["model"])
    for name, value in saved[0]["model"].items():
        assert torch.equal(value, saved[1]["model"][name]), name
    first = torch.load(os.path.join(G.T.checkpoint_dir(conf), "checkpoint_iter00000002.pt"), weights_only=True)
    assert any(not torch.equal(v, first["model"][k]) for k, v in saved[0]["model"].items())        # it trained


# ---------------------------------------------------------------------------
# the command
def test_restore_command_scores_against_the_reference_files(G, tmp_path, capsys):
    """restore.py --reference, in this process: the lines carry the PSNR / SSIM of the files written against the
    references, --batch-images and an ensemble print what the plain runs print, a mis-sized reference stops the
    command before the model is built."""
    import re
    from PIL import Image
    from tests.test_restore_ref import _cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    yaml_path = os.path.join(root, "experiment_conf", "example.yaml")       # a one-channel model, no checkpoint
    src, ref, dst = tmp_path / "in", tmp_path / "ref", tmp_path / "out"
    src.mkdir()
    ref.mkdir()
    clean = {"a": patch_ref.picture(1, 37, 53, 1)[:, :, 0], "b": patch_ref.picture(2, 48, 40, 1)[:, :, 0]}
    rs = np.random.RandomState(9)
    for name, img in clean.items():
        Image.fromarray(img).save(ref / f"{name}.png")
        Image.fromarray(np.clip(img.astype(np.int64) + rs.randint(-12, 13, img.shape), 0, 255).astype(np.uint8)).save(
            src / f"{name}.png")
    base = ["-yaml_path", yaml_path, "--input", str(src), "--output", str(dst), "--reference", str(ref), "--tile", "64",
            "--halo", "16"]
    cli = _cli()
    outs = {}
    for key, extra in (("plain", []), ("ssim", ["--ssim"]), ("batch", ["--ssim", "--batch-images"])):
        torch.manual_seed(3)
        cli.main(base + extra)
        outs[key] = capsys.readouterr().out
    assert "SSIM" not in outs["plain"] and outs["batch"] == outs["ssim"]
    lines = [ln for ln in outs["ssim"].splitlines() if " -> " in ln]
    assert len(lines) == 2
    psnrs = []
    for line, name in zip(lines, ("a", "b")):
        m = re.search(r"  reference (\S+)  PSNR (\d+\.\d{4}) dB  SSIM (-?\d\.\d{4})$", line)
        assert m and m.group(1) == str(ref / f"{name}.png"), line
        written = np.array(Image.open(dst / f"{name}.png"))
        psnrs.append(G.R.psnr_u8(written, clean[name]))
        assert m.group(2) == f"{psnrs[-1]:.4f}"
        assert m.group(3) == f"{G.R.ssim_u8(written[:, :, None], clean[name][:, :, None]):.4f}"
    assert outs["ssim"].splitlines()[-2] == f"mean PSNR over 2 image(s): {float(np.mean(psnrs)):.4f} dB"
    torch.manual_seed(3)
    cli.main(base + ["--ensemble-modes", "0,1"])
    assert capsys.readouterr().out.count("PSNR") == 3
    Image.fromarray(np.ascontiguousarray(clean["b"][:, :39])).save(ref / "b.png")
    with pytest.raises(SystemExit, match=r"b\.png is 48x39x1"):
        cli.main(base)
    capsys.readouterr()
