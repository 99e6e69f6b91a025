"""CPU: the amp mode's host side -- train()'s (amp, mixed_precision_type) mapping, its gin keywords, and the per-parameter policy."""
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_amp_settings_map_to_an_autocast_dtype_as_accelerate_does():
    import hidvae_amd  # noqa: F401
    from hidvae_amd.train_hidvae import amp_dtype
    assert amp_dtype(True, "bf16") is torch.bfloat16
    assert amp_dtype(True, "no") is None
    for mpt in ("no", "fp16", "bf16", "fp8"):
        assert amp_dtype(False, mpt) is None
    for mpt in ("fp16", "fp8"):
        with pytest.raises(NotImplementedError, match='"bf16"'):
            amp_dtype(True, mpt)
    with pytest.raises(ValueError):
        amp_dtype(True, "int8")


def test_train_refuses_fp16_amp_before_touching_a_device():
    import hidvae_amd  # noqa: F401
    from hidvae_amd.train_hidvae import train
    with pytest.raises(NotImplementedError, match="bf16"):
        train(amp=True)  # the reference's default mixed_precision_type is "fp16"


def test_gin_binds_the_amp_keywords():
    import inspect
    import hidvae_amd  # noqa: F401
    from hidvae_amd import gin_compat as gin
    from hidvae_amd.train_hidvae import train
    gin.clear_config()
    try:
        gin.parse_config_file(os.path.join(GOLDEN, "h_rqvae_amazon.gin"),
                              import_aliases={"data.tags_processed": "hidvae_amd.data.items", "modules.quantize": "hidvae_amd.modules.quantize"})
        gin.parse_config('train.amp = True\ntrain.mixed_precision_type = "bf16"\n')
        b = gin.bindings("train")
        assert b["amp"] is True and b["mixed_precision_type"] == "bf16"
        assert {"amp", "mixed_precision_type"} <= set(inspect.signature(train.__wrapped__).parameters)
    finally:
        gin.clear_config()


def _amazon_model():
    from hidvae_amd.modules.h_rqvae import HRqVae
    from hidvae_amd.modules.quantize import QuantizeForwardMode
    return HRqVae(input_dim=768, embed_dim=32, hidden_dims=[512, 256, 128], codebook_size=256, codebook_kmeans_init=False,
                  codebook_normalize=True, codebook_mode=QuantizeForwardMode.ROTATION_TRICK, n_layers=3, n_cat_features=0,
                  tag_class_counts=[38, 168, 348], tag_embed_dim=768, use_focal_loss=True, dropout_rate=0.4)


def test_default_policy_names_only_linear_weights_of_the_tagged_model():
    import hidvae_amd  # noqa: F401
    m = _amazon_model()
    names = m.amp_bf16_parameters()
    assert len(names) == len(set(names))
    mods = dict(m.named_modules())
    sd = m.state_dict()
    for n in names:
        assert n in sd and n.endswith(".weight"), n
        assert isinstance(mods[n[: -len(".weight")]], torch.nn.Linear), n
    want = {"encoder.mlp.0.weight", "encoder.mlp.2.weight", "decoder.mlp.4.weight", "decoder.mlp.6.weight"}
    want |= {f"tag_projectors.{i}.{k}.weight" for i in range(3) for k in (0, 4)}
    for i in (1, 2):
        want |= {f"tag_predictors.{i}.{n}.weight" for n in ("feature_extractor.0", "residual_block1.0", "residual_block1.4", "residual_block2.0",
                                                             "residual_block2.4", "classifier.0", "classifier.4", "classifier.7")}
    assert set(names) == want
    # fp32 at every batch size: the four layers around the bottleneck, level 0's predictor, every gate, the quantiser
    for n in ("encoder.mlp.4.weight", "encoder.mlp.6.weight", "decoder.mlp.0.weight", "decoder.mlp.2.weight",
              "tag_predictors.0.feature_extractor.0.weight", "tag_predictors.1.attention.0.weight", "layers.0.embedding.weight"):
        assert n not in names


def test_amp_off_sees_no_bf16_precision():
    import hidvae_amd  # noqa: F401
    from hidvae_amd import ops
    m = _amazon_model()
    m._mark_amp_parameters()
    w = m.encoder.mlp[0].weight
    assert ops.precision_of(w) == "fp32"  # outside an amp scope
    with ops.amp_scope(True):
        assert ops.precision_of(w) == "bf16" and ops.precision_of(m.encoder.mlp[4].weight) == "fp32"
        assert not torch.is_autocast_enabled("cuda")
    with ops.amp_scope(False):
        assert ops.precision_of(w) == "fp32"
    assert ops.precision_of(w) == "fp32"
