"""The ``datasets.val`` section of the YAML, without a GPU: for each of the five validation configurations (noise,
pairs, ``scale``, ``jpeg_quality``, ``bayer``) and for configurations with two selecting keys, the arguments
training.create_val_dataset returns, against literal dicts, and the validator training.val_check picks for them, by
identity.  The precedence is jpeg_quality, then bayer, then scale, then TestPairsCSV, then noise.  No model runs."""
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
    ("noise-defaults", "clean", {}, "TestImagesCSV", dict(sigma=25.0, factor=16), "validate"),
    ("noise", "clean", dict(sigma=15, factor="8", tile=64, metric="psnr_y"), "TestImagesCSV", dict(sigma=15.0, factor=8),
     "validate"),
    ("noise-synthetic", "synthetic", dict(sigma=50.0), "SyntheticTestImages", dict(sigma=50.0, factor=16), "validate"),
    ("pairs-defaults", "pairs", {}, "TestPairsCSV", dict(factor=16), "validate_pairs"),
    ("pairs", "pairs", dict(tile="64", halo=16, micro_batch=4, metric="psnr_y", factor=32, sigma=15.0, shave=2),
     "TestPairsCSV", dict(tile=64, halo=16, micro_batch=4, metric="psnr_y", factor=32), "validate_pairs"),
    ("scale-defaults", "clean", dict(scale=4), "TestImagesCSV", dict(scale=4, factor=16), "validate_sr"),
    ("scale", "clean", dict(scale="3", shave=0, tile=64, halo=16, micro_batch=2, metric="psnr", subsampling=2, fill="zero"),
     "TestImagesCSV", dict(scale=3, shave=0, tile=64, halo=16, micro_batch=2, metric="psnr", factor=16), "validate_sr"),
    ("jpeg-defaults", "clean", dict(jpeg_quality=10), "TestImagesCSV", dict(jpeg_quality=10, factor=16), "validate_car"),
    ("jpeg", "clean", dict(jpeg_quality="40", subsampling=2, tile=64, halo=16, micro_batch=8, metric="psnrb", shave=3),
     "TestImagesCSV", dict(jpeg_quality=40, subsampling=2, tile=64, halo=16, micro_batch=8, metric="psnrb", factor=16),
     "validate_car"),
    ("bayer-defaults", "clean", dict(bayer="rggb"), "TestImagesCSV", dict(bayer="rggb", factor=16), "validate_demosaic"),
    ("bayer", "clean", dict(bayer="gbrg", fill="bilinear", shave="4", tile=64, halo=16, micro_batch=1, metric="ssim",
                            factor=8, subsampling=2),
     "TestImagesCSV", dict(bayer="gbrg", fill="bilinear", shave=4, tile=64, halo=16, micro_batch=1, metric="ssim", factor=8),
     "validate_demosaic"),
    # two selecting keys: jpeg_quality, then bayer, then scale; a key of clean pictures does not select on other sets
    ("jpeg-over-bayer", "clean", dict(jpeg_quality=10, bayer="rggb", fill="zero", shave=2, metric="psnrb"),
     "TestImagesCSV", dict(jpeg_quality=10, metric="psnrb", factor=16), "validate_car"),
    ("jpeg-over-scale", "clean", dict(jpeg_quality=10, scale=2, shave=2), "TestImagesCSV", dict(jpeg_quality=10, factor=16),
     "validate_car"),
    ("bayer-over-scale", "clean", dict(bayer="bggr", scale=2, shave=2, metric="ssim"), "TestImagesCSV",
     dict(bayer="bggr", shave=2, metric="ssim", factor=16), "validate_demosaic"),
    ("all-three", "clean", dict(scale=2, bayer="grbg", jpeg_quality=90), "TestImagesCSV", dict(jpeg_quality=90, factor=16),
     "validate_car"),
    ("pairs-over-scale", "pairs", dict(scale=2, jpeg_quality=10, bayer="rggb"), "TestPairsCSV", dict(factor=16),
     "validate_pairs"),
    ("synthetic-over-scale", "synthetic", dict(scale=2, jpeg_quality=10), "SyntheticTestImages", dict(sigma=25.0, factor=16),
     "validate"),
]


@pytest.mark.parametrize("which,extra,cls,want,check", [c[1:] for c in CONFIGS], ids=[c[0] for c in CONFIGS])
def test_the_arguments_and_the_validator_of_a_validation_config(sets, which, extra, cls, want, check):
    val_set, val_args = T.create_val_dataset(dict(datasets=dict(val=dict(sets[which], **extra))))
    assert type(val_set) is getattr(T, cls)
    assert val_args == want and all(type(val_args[k]) is type(want[k]) for k in want)
    assert T.val_check(val_set, val_args) is getattr(T, check)


def test_no_validation_section_and_an_unknown_type():
    assert T.create_val_dataset({}) == (None, {}) and T.create_val_dataset(dict(datasets=dict(val=None))) == (None, {})
    with pytest.raises(ValueError, match="Validation dataset Nope is not found."):
        T.create_val_dataset(dict(datasets=dict(val=dict(type="Nope"))))


# the refusals, in the order they are raised: the selecting key's value, the other names, then the metric
REFUSALS = [
    ("clean", dict(bayer="rgbg", fill="linear", metric="psnrb"), r"datasets.val.bayer is one of \('rggb', 'grbg', 'gbrg', 'bggr'\), got 'rgbg'"),
    ("clean", dict(bayer="rggb", fill="linear", metric="psnrb"), r"datasets.val.fill is one of \('zero', 'bilinear', 'malvar'\), got 'linear'"),
    ("clean", dict(bayer="rggb", metric="psnrb"), r"datasets.val.metric is one of \('psnr', 'psnr_y', 'ssim'\), got 'psnrb'"),
    ("clean", dict(jpeg_quality=10, metric="ssim"), r"datasets.val.metric is one of \('psnr', 'psnr_y', 'psnrb'\), got 'ssim'"),
    ("clean", dict(scale=2, metric="ssim"), r"datasets.val.metric is one of \('psnr', 'psnr_y'\), got 'ssim'"),
    ("pairs", dict(metric="ssim"), r"datasets.val.metric is one of \('psnr', 'psnr_y'\), got 'ssim'"),
]


@pytest.mark.parametrize("which,extra,message", REFUSALS)
def test_the_refusals_of_a_validation_config(sets, which, extra, message):
    with pytest.raises(ValueError, match=message):
        T.create_val_dataset(dict(datasets=dict(val=dict(sets[which], **extra))))


def test_validate_demosaic_lifts_a_2d_picture_as_its_siblings_do_and_the_protocol_refuses_it(monkeypatch):
    import numpy as np
    from irdu_amd import kernels

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(kernels, "_launch", no_launch)
    for gray in (np.zeros((20, 24), np.uint8), np.zeros((20, 24), np.float32)):
        with pytest.raises(ValueError, match=r"evaluate_demosaic: image 0 is \(20, 24, 1\); the protocol takes clean R, G, B"):
            T.validate_demosaic(lambda x: x, [gray], device="cpu")
