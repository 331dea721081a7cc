"""The ``datasets.val`` section of the YAML with a ``blur`` key, without a GPU: the arguments
training.create_val_dataset returns, against literal dicts, and the validator training.val_check picks for them, by
identity.  The deblurring row comes after jpeg_quality, bayer and scale and before the pairs row; its float key is
``noise_sigma`` -- ``sigma`` stays the noise protocol's and is ignored here.  No model runs."""
import pytest

from irdu_amd import training as T


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = tmp_path_factory.mktemp("val")
    (d / "clean.csv").write_text("index,path\n0,a.png\n")
    (d / "pairs.csv").write_text("index,path,target_path\n0,a.png,b.png\n")
    return dict(clean=dict(type="TestImagesCSV", dataset_args=dict(csv_path=str(d / "clean.csv"), root_folder=str(d))),
                pairs=dict(type="TestPairsCSV", dataset_args=dict(csv_path=str(d / "pairs.csv"), root_folder=str(d))),
                synthetic=dict(type="SyntheticTestImages", dataset_args=dict(n_images=2)))


# (id, the dataset, the other keys of datasets.val, the dataset's class, the arguments, the validator)
CONFIGS = [
    ("blur-defaults", "clean", dict(blur="gaussian:25:1.6"), "TestImagesCSV", dict(blur="gaussian:25:1.6", factor=16),
     "validate_deblur"),
    ("blur", "clean", dict(blur="motion:15:30", boundary="reflect", noise_sigma="2.55", shave="4", tile=64, halo=16,
                           micro_batch=1, metric="ssim", factor=8, subsampling=2, fill="zero", sigma=15.0),
     "TestImagesCSV", dict(blur="motion:15:30", boundary="reflect", noise_sigma=2.55, shave=4, tile=64, halo=16,
                           micro_batch=1, metric="ssim", factor=8), "validate_deblur"),
    ("blur-integer-noise", "clean", dict(blur="box:5", noise_sigma=2), "TestImagesCSV",
     dict(blur="box:5", noise_sigma=2.0, factor=16), "validate_deblur"),
    # two selecting keys: jpeg_quality, then bayer, then scale, then blur; a key of clean pictures does not select on
    # other sets
    ("jpeg-over-blur", "clean", dict(jpeg_quality=10, blur="box:3", boundary="wrap", noise_sigma=1.0, shave=2),
     "TestImagesCSV", dict(jpeg_quality=10, factor=16), "validate_car"),
    ("bayer-over-blur", "clean", dict(bayer="bggr", blur="box:3", noise_sigma=1.0, shave=2), "TestImagesCSV",
     dict(bayer="bggr", shave=2, factor=16), "validate_demosaic"),
    ("scale-over-blur", "clean", dict(scale=2, blur="box:3", boundary="reflect", noise_sigma=1.0), "TestImagesCSV",
     dict(scale=2, factor=16), "validate_sr"),
    ("all-four", "clean", dict(blur="box:3", scale=2, bayer="grbg", jpeg_quality=90), "TestImagesCSV",
     dict(jpeg_quality=90, factor=16), "validate_car"),
    ("pairs-over-blur", "pairs", dict(blur="box:3", noise_sigma=1.0), "TestPairsCSV", dict(factor=16), "validate_pairs"),
    ("synthetic-over-blur", "synthetic", dict(blur="box:3", noise_sigma=1.0), "SyntheticTestImages",
     dict(sigma=25.0, factor=16), "validate"),
    # the rows before it give what they gave: no float key reaches them
    ("scale-ignores-noise-sigma", "clean", dict(scale=3, noise_sigma=2.0, boundary="wrap"), "TestImagesCSV",
     dict(scale=3, factor=16), "validate_sr"),
]


@pytest.mark.parametrize("which,extra,cls,want,check", [c[1:] for c in CONFIGS], ids=[c[0] for c in CONFIGS])
def test_the_arguments_and_the_validator_of_a_validation_config(sets, which, extra, cls, want, check):
    val_set, val_args = T.create_val_dataset(dict(datasets=dict(val=dict(sets[which], **extra))))
    assert type(val_set) is getattr(T, cls)
    assert val_args == want and all(type(val_args[k]) is type(want[k]) for k in want)
    assert T.val_check(val_set, val_args) is getattr(T, check)


def test_the_order_of_the_rows():
    keys = [p.key for p in T._VAL_PROTOCOLS]
    assert keys == ["jpeg_quality", "bayer", "scale", "blur", None]
    assert [p.float_keys for p in T._VAL_PROTOCOLS] == [(), (), (), ("noise_sigma",), ()]
    assert all("sigma" not in p.int_keys + p.float_keys + tuple(p.choices) for p in T._VAL_PROTOCOLS)


# the refusals, in the order they are raised: the other names, then the metric, then the spec itself
REFUSALS = [
    ("clean", dict(blur="gauss:3:1", boundary="circular", metric="psnrb"),
     r"datasets.val.boundary is one of \('wrap', 'replicate', 'reflect'\), got 'circular'"),
    ("clean", dict(blur="gauss:3:1", metric="psnrb"), r"datasets.val.metric is one of \('psnr', 'psnr_y', 'ssim'\), got 'psnrb'"),
    ("clean", dict(blur="gauss:3:1"), r"parse_blur_spec: a blur spec is gaussian:SIDE:SIGMA"),
    ("clean", dict(blur="box:4"), r"box_kernel: the side is an odd integer of 1..31, got 4"),
    ("clean", dict(blur=5), r"datasets.val.blur is a kernel spec string"),
    ("clean", dict(blur=[[1]]), r"datasets.val.blur is a kernel spec string"),
    ("clean", dict(blur="box:3", noise_sigma="much"), r"could not convert string to float"),
    ("clean", dict(blur="box:3", shave="x"), r"invalid literal for int"),
]


@pytest.mark.parametrize("which,extra,message", REFUSALS)
def test_the_refusals_of_a_validation_config(sets, which, extra, message):
    with pytest.raises(ValueError, match=message):
        T.create_val_dataset(dict(datasets=dict(val=dict(sets[which], **extra))))


def test_validate_deblur_hands_its_arguments_to_evaluate_deblur(monkeypatch):
    import numpy as np
    from irdu_amd import restore
    seen = {}

    def evaluate(model, images, **kw):
        seen.update(kw, n=len(images), dtypes={a.dtype for a in images}, shapes=[a.shape for a in images])
        return {kw["metrics"][0]: (1.5, [1.0, 2.0])}

    monkeypatch.setattr(restore, "evaluate_deblur", evaluate)
    pics = [np.zeros((20, 24), np.float32), np.zeros((12, 12, 3), np.uint8)]
    got = T.validate_deblur(None, pics, "box:3", boundary="reflect", noise_sigma=2.0, shave=1, factor=8, device="cpu",
                            metric="ssim", tile=64)
    assert got == 1.5
    assert seen == dict(kernel="box:3", boundary="reflect", noise_sigma=2.0, seed=2204, shave=1, factor=8, device="cpu",
                        metrics=("ssim",), tile=64, n=2, dtypes={np.dtype(np.uint8)}, shapes=[(20, 24, 1), (12, 12, 3)])
