#!/usr/bin/env python3
"""Generate tests/golden/checkpoint_reference_iter13.pt: the checkpoint the REFERENCE writes back after resuming from a file of
ours (reference train_hidvae.py:621-638 reads and resumes, :1161-1171 writes), for tests/test_checkpoint_cpu.py.
    python tests/golden/make_golden_checkpoint.py <reference tree>
The reference side runs in a process of its own without hidvae_amd (stub gin, the spelling alias, TORCHDYNAMO_DISABLE=1, as in
make_golden.py); its model load is strict and its optimizer is torch's own AdamW, so a file it writes proves the interchange."""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

REFERENCE_SIDE = r'''
import sys, types
sys.path.insert(0, sys.argv[1])
g = types.ModuleType("gin"); g.configurable = lambda f=None, **k: f if f is not None else (lambda h: h); g.constants_from_enum = lambda c: c
sys.modules["gin"] = g
import torch
import modules.loss as L
L.CategoricalReconstuctionLoss = L.CategoricalReconstructionLoss
from modules.h_rqvae import HRqVae
from modules.quantize import QuantizeForwardMode
assert "hidvae_amd" not in sys.modules
src, dst = sys.argv[2], sys.argv[3]
state = torch.load(src, map_location="cpu", weights_only=False)           # train_hidvae.py:624
cfg = state["model_config"]
assert cfg["codebook_mode"] is QuantizeForwardMode.ROTATION_TRICK, cfg["codebook_mode"]
model = HRqVae(**cfg)
model.load_state_dict(state["model"])                                      # strict: the key contract, both directions
lr, wd, pwd = 2.8e-4, 0.015, 0.02
groups = [{"params": list(model.encoder.parameters()) + list(model.decoder.parameters()), "lr": lr, "weight_decay": wd},
          {"params": [p for layer in model.layers for p in layer.parameters()], "lr": lr, "weight_decay": wd}]
for i in range(cfg["n_layers"]):
    groups.append({"params": model.tag_predictors[i].parameters(), "lr": lr * (1 + i * 0.1), "weight_decay": pwd / (1 + i * 0.2)})
    groups.append({"params": model.tag_projectors[i].parameters(), "lr": lr * (1 + i * 0.1), "weight_decay": pwd / (1 + i * 0.2)})
opt = torch.optim.AdamW(groups)
opt.load_state_dict(state["optimizer"])                                    # train_hidvae.py:625
start_iter = state["iter"] + 1
sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=1000, eta_min=1e-6, last_epoch=start_iter - 1)   # :638
for p in model.parameters():
    p.grad = torch.full_like(p, 1e-3)
opt.step(); sched.step()
out = {"iter": start_iter, "model": model.state_dict(), "model_config": model.config, "optimizer": opt.state_dict(),
       "accuracy": 0.7, "rqvae_loss": 0.1, "sem_id_repetition_rate": 0.01}  # :1161-1169 (config pickles the module too, SURVEY Q11)
torch.save(out, dst)
print("reference-side ok", len(state["model"]), float(list(opt.state.values())[0]["step"]))
'''


def main():
    from tests.test_checkpoint_cpu import GOLDEN, write_ours
    ref = os.path.abspath(sys.argv[1])
    with tempfile.TemporaryDirectory() as tmp:
        ours = os.path.join(tmp, "ours.pt")
        write_ours(ours)
        env = {**os.environ, "TORCHDYNAMO_DISABLE": "1"}
        out = subprocess.run([sys.executable, "-c", REFERENCE_SIDE, ref, ours, GOLDEN], capture_output=True, text=True, timeout=600,
                             env=env, cwd=tmp)
    if out.returncode != 0 or "reference-side ok" not in out.stdout:
        sys.exit(out.stderr[-3000:])
    print(out.stdout.strip(), "->", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
