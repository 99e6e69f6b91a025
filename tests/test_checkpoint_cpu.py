"""CPU: checkpoint interchange with the reference (reference train_hidvae.py:621-628 reads, :1161-1171 writes).

The "optimizer" entry is a genuine torch.optim.AdamW.state_dict(); the one pickled object of the file (the QuantizeForwardMode enum
in model_config) is named by the reference's module path, so a file written here loads in an environment WITHOUT hidvae_amd and a
file written by the reference loads here."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import hidvae_amd  # noqa: F401
from hidvae_amd.optim import HidvaeAdamW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(input_dim=40, embed_dim=32, hidden_dims=[64, 48], codebook_size=16, codebook_kmeans_init=False, codebook_normalize=True,
           n_layers=2, n_cat_features=0, tag_class_counts=[5, 7], tag_embed_dim=24, use_focal_loss=True,
           focal_loss_params={"gamma_0": 2.7, "alpha_0": 0.24}, dropout_rate=0.4)


def mirror_model():
    from hidvae_amd.modules.h_rqvae import HRqVae
    from hidvae_amd.modules.quantize import QuantizeForwardMode
    torch.manual_seed(3)
    return HRqVae(codebook_mode=QuantizeForwardMode.ROTATION_TRICK, **CFG)


def groups_of(m, lr=2.8e-4, wd=0.015, pwd=0.02):
    """reference train_hidvae.py:533-563"""
    g = [{"params": list(m.encoder.parameters()) + list(m.decoder.parameters()), "lr": lr, "weight_decay": wd},
         {"params": [p for layer in m.layers for p in layer.parameters()], "lr": lr, "weight_decay": wd}]
    for i in range(m.n_layers):
        g.append({"params": list(m.tag_predictors[i].parameters()), "lr": lr * (1 + 0.1 * i), "weight_decay": pwd / (1 + 0.2 * i)})
        g.append({"params": list(m.tag_projectors[i].parameters()), "lr": lr * (1 + 0.1 * i), "weight_decay": pwd / (1 + 0.2 * i)})
    return g


def test_optimizer_state_is_a_torch_adamw_state_dict_both_ways():
    m = mirror_model()
    opt = HidvaeAdamW(groups_of(m), cosine=(1000, 1e-6)).prepare()
    g = torch.Generator().manual_seed(0)
    opt._m.copy_(torch.randn(opt._m.shape, generator=g) * 1e-3)
    opt._v.copy_(torch.rand(opt._v.shape, generator=g) * 1e-6)
    opt.step_dev[0] = 7
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and len(sd["param_groups"]) == 2 + 2 * m.n_layers
    n_params = sum(len(grp["params"]) for grp in sd["param_groups"])
    assert sorted(sd["state"]) == list(range(n_params))
    # -> torch's own optimizer, built with the reference's groups, takes it
    m2 = mirror_model()
    ref = torch.optim.AdamW(groups_of(m2))
    ref.load_state_dict(sd)
    flat = [p for grp in ref.param_groups for p in grp["params"]]
    off = 0
    for p in flat:
        st = ref.state[p]
        n = p.numel()
        assert float(st["step"]) == 7.0
        assert torch.equal(st["exp_avg"].reshape(-1), opt._m[off:off + n]) and torch.equal(st["exp_avg_sq"].reshape(-1), opt._v[off:off + n])
        off += n
    want_lr = 1e-6 + (2.8e-4 - 1e-6) * (1 + math.cos(math.pi * 7 / 1000)) / 2
    assert abs(ref.param_groups[0]["lr"] - want_lr) < 1e-12 and ref.param_groups[0]["initial_lr"] == 2.8e-4
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(ref, T_max=1000, eta_min=1e-6, last_epoch=6)  # the reference's resume (:638)
    for p in flat:
        p.grad = torch.ones_like(p) * 1e-3
    ref.step()
    sched.step()
    # <- and a state written by torch's optimizer loads into the fused one
    sd2 = ref.state_dict()
    m3 = mirror_model()
    opt3 = HidvaeAdamW(groups_of(m3), cosine=(1000, 1e-6)).prepare()
    assert opt3.load_state_dict(sd2) is True
    assert opt3.step_dev.tolist() == [8, 0]
    off = 0
    for p in flat:
        n = p.numel()
        assert torch.equal(ref.state[p]["exp_avg"].reshape(-1), opt3._m[off:off + n])
        assert torch.equal(ref.state[p]["exp_avg_sq"].reshape(-1), opt3._v[off:off + n])
        off += n
    assert opt3.param_groups[2]["lr"] == 2.8e-4 and abs(opt3.param_groups[4]["lr"] - 2.8e-4 * 1.1) < 1e-15  # base rates, not scheduled ones
    # the round-1 private layout is still read
    opt4 = HidvaeAdamW(groups_of(mirror_model()), cosine=(1000, 1e-6)).prepare()
    assert opt4.load_state_dict(opt.flat_state()) is True and torch.equal(opt4._m, opt._m) and int(opt4.step_dev[0]) == 7


def test_resume_without_optimizer_state_restarts_bias_correction_but_not_the_schedule():
    opt = HidvaeAdamW(groups_of(mirror_model()), cosine=(1000, 1e-6), start_step=500).prepare()
    assert opt.load_state_dict({"state": {}, "param_groups": torch.optim.AdamW(groups_of(mirror_model())).state_dict()["param_groups"]}) is False
    assert opt.step_dev.tolist() == [0, 500]
    assert abs(opt.current_lr() - (1e-6 + (2.8e-4 - 1e-6) * 0.5)) < 1e-9  # cosine at half of T_max
    with pytest.raises(ValueError):
        opt.load_state_dict({"state": {}, "param_groups": [{"params": [0]}]})


def test_flat_state_round_trips_into_an_optimizer_with_a_first_bucket():
    """the flat moment layout leads with the data-parallel first bucket, so a flat state must be scattered parameter by
    parameter (positional copies put Adam moments on the wrong parameters; sizes match, nothing raised)"""
    m = mirror_model()
    opt = HidvaeAdamW(groups_of(m), cosine=(1000, 1e-6)).prepare()
    opt._m.copy_(torch.arange(opt._m.numel(), dtype=torch.float32))
    opt._v.copy_(torch.arange(opt._v.numel(), dtype=torch.float32) * 2)
    opt.step_dev[0] = 9
    per_param = {id(p): opt._m[o:o + n].clone() for p, (o, n) in ((p, opt._slots()[id(p)]) for p in opt._params)}
    # same model object, another optimizer whose flat order leads with the decoder's last two layers
    first = list(m.decoder.parameters())[-2:]
    opt2 = HidvaeAdamW(groups_of(m), cosine=(1000, 1e-6), first_bucket=first).prepare()
    assert opt2.n_first == 2 and opt2._params[0] is first[0] and opt2._params[0] is not opt._params[0]
    fs = opt.flat_state()
    assert opt2.load_state_dict(fs) is True
    for p in opt2._params:
        o, n = opt2._slots()[id(p)]
        assert torch.equal(opt2._m[o:o + n], per_param[id(p)]), "moment landed on another parameter"
    # and back: a state written WITH a first bucket loads into a plain optimizer
    opt3 = HidvaeAdamW(groups_of(m), cosine=(1000, 1e-6)).prepare()
    assert opt3.load_state_dict(opt2.flat_state()) is True and torch.equal(opt3._m, opt._m) and torch.equal(opt3._v, opt._v)
    # a round-1 file (no order recorded) is in group order
    legacy = {k: v for k, v in fs.items() if k not in ("order", "numels", "schedule_offset")}
    opt4 = HidvaeAdamW(groups_of(m), cosine=(1000, 1e-6), first_bucket=first).prepare()
    assert opt4.load_state_dict(legacy) is True
    for p in opt4._params:
        o, n = opt4._slots()[id(p)]
        assert torch.equal(opt4._m[o:o + n], per_param[id(p)])
    bad = dict(fs, numels=[1] + fs["numels"][1:])
    with pytest.raises(ValueError):
        opt4.load_state_dict(bad)


def test_resuming_twice_keeps_the_schedule_position():
    """state_dict() dropped the schedule offset of a run resumed without optimizer state"""
    opt = HidvaeAdamW(groups_of(mirror_model()), cosine=(1000, 1e-6)).prepare()
    opt.restart_without_state(500)
    opt.step_dev[0] = 3  # three optimizer steps after the restart
    opt._m.fill_(0.5)
    sd = opt.state_dict()
    opt2 = HidvaeAdamW(groups_of(mirror_model()), cosine=(1000, 1e-6)).prepare()
    assert opt2.load_state_dict(sd) is True
    assert opt2.step_dev.tolist() == [3, 500] and abs(opt2.current_lr() - opt.current_lr()) < 1e-12
    torch.optim.AdamW(groups_of(mirror_model())).load_state_dict(sd)  # the extra key does not disturb torch's own loader


GOLDEN = os.path.join(ROOT, "tests", "golden", "checkpoint_reference_iter13.pt")
# What the reference does with a file of ours (tests/golden/make_golden_checkpoint.py runs it and keeps what the reference wrote back):
# torch.load in an environment without hidvae_amd (train_hidvae.py:624), HRqVae(**model_config) + a STRICT load_state_dict, its
# AdamW groups (:533-563) + optimizer.load_state_dict (:625), the resume schedule (:638), one step on constant 1e-3 gradients, save
# (:1161-1169).  The file it wrote holds its own state_dict and AdamW state, so the same checks need only that file.
WITHOUT_PACKAGE = r'''
import json, sys
import torch
assert "hidvae_amd" not in sys.modules
from modules.quantize import QuantizeForwardMode
state = torch.load(sys.argv[1], map_location="cpu", weights_only=False)
assert "hidvae_amd" not in sys.modules
assert state["model_config"]["codebook_mode"] is QuantizeForwardMode.ROTATION_TRICK, state["model_config"]["codebook_mode"]
print(json.dumps({"iter": state["iter"], "model": [[k, list(v.shape), str(v.dtype)] for k, v in state["model"].items()],
                  "groups": [len(g["params"]) for g in state["optimizer"]["param_groups"]], "state": sorted(state["optimizer"]["state"])}))
'''
# the reference's enum (modules/quantize.py), all a file of ours needs from the reference environment to unpickle
STAND_IN_QUANTIZE = "from enum import Enum\n\n\nclass QuantizeForwardMode(Enum):\n    GUMBEL_SOFTMAX = 1\n    STE = 2\n    ROTATION_TRICK = 3\n"


def write_ours(path):
    """-> (model, optimizer) of the checkpoint written to `path` (iter 12, seeded Adam moments)"""
    from hidvae_amd.checkpoint import save_checkpoint
    m = mirror_model()
    opt = HidvaeAdamW(groups_of(m), cosine=(1000, 1e-6)).prepare()
    g = torch.Generator().manual_seed(1)
    opt._m.copy_(torch.randn(opt._m.shape, generator=g) * 1e-3)
    opt._v.copy_(torch.rand(opt._v.shape, generator=g) * 1e-6)
    opt.step_dev[0] = 12
    save_checkpoint({"iter": 12, "model": m.state_dict(), "model_config": m.config, "optimizer": opt.state_dict(), "accuracy": 0.65,
                     "rqvae_loss": 0.2, "sem_id_repetition_rate": 0.02}, path)
    return m, opt


def test_checkpoint_round_trip_through_the_reference(tmp_path):
    from hidvae_amd.checkpoint import load_checkpoint
    ours = str(tmp_path / "ours.pt")
    m, opt = write_ours(ours)
    from hidvae_amd.modules.quantize import QuantizeForwardMode
    assert QuantizeForwardMode.__module__ == "hidvae_amd.modules.quantize" and "modules.quantize" not in sys.modules  # aliases were temporary
    # our file in an environment WITHOUT hidvae_amd, where modules.quantize is the reference's
    (tmp_path / "modules").mkdir()
    (tmp_path / "modules" / "__init__.py").write_text("")
    (tmp_path / "modules" / "quantize.py").write_text(STAND_IN_QUANTIZE)
    env = {**os.environ, "TORCHDYNAMO_DISABLE": "1", "PYTHONPATH": str(tmp_path)}
    out = subprocess.run([sys.executable, "-c", WITHOUT_PACKAGE, ours], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    seen = json.loads(out.stdout.strip().splitlines()[-1])
    # the file the REFERENCE wrote back from the same file of ours (its own torch optimizer, its own pickled enum and module) loads here
    state = load_checkpoint(GOLDEN, map_location="cpu")
    # the reference's strict load_state_dict and AdamW.load_state_dict accept exactly its own keys, shapes and group sizes
    assert seen["iter"] == 12
    assert seen["model"] == [[k, list(v.shape), str(v.dtype)] for k, v in state["model"].items()]
    assert seen["groups"] == [len(g["params"]) for g in state["optimizer"]["param_groups"]]
    assert seen["state"] == list(range(sum(seen["groups"])))
    assert state["iter"] == 13 and state["model_config"]["codebook_mode"] is QuantizeForwardMode.ROTATION_TRICK
    assert "self" not in state["model_config"]
    m2 = mirror_model()
    m2.load_state_dict(state["model"])
    assert list(m2.state_dict()) == list(state["model"])
    opt2 = HidvaeAdamW(groups_of(m2), cosine=(1000, 1e-6)).prepare()
    assert opt2.load_state_dict(state["optimizer"]) is True
    assert int(opt2.step_dev[0]) == 13
    # one torch AdamW step on constant gradients from our moments: m' = 0.9 m + 0.1 g, v' = 0.999 v + 0.001 g^2
    assert torch.allclose(opt2._m, 0.9 * opt._m + 0.1 * 1e-3, rtol=1e-5, atol=1e-9)
    assert torch.allclose(opt2._v, 0.999 * opt._v + 0.001 * 1e-6, rtol=1e-5, atol=1e-12)
