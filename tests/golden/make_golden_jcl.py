"""Generates tests/golden/jcl_*.npz: JointCodebookLoss of the reference (quantization/prediction.py:9-172) on seeded
inputs -- its initial state, the loss, and the gradients w.r.t. every parameter and the predictor.  Runs only in
the build container (imports the reference); the fixtures are data.

    python tests/golden/make_golden_jcl.py [NAME ...]       (no name: every fixture)
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.modules.setdefault("h5py", types.ModuleType("h5py"))
sys.path.insert(0, "/root/reference")
import quantization as refq  # noqa: E402


def pad_whole_frames(flat):
    flat[::7] = -100                          # padding frames: all codebooks negative (:150-154)


def pad_partial(flat):
    """single negatives in codebooks 0, 2 and 4 of different frames (later codebooks valid: the clamped entry 0 of :44-50
    is gathered and trained), and every eleventh frame wholly negative"""
    flat[::11] = -100
    flat[3, 0] = -100
    flat[8, 2] = -100
    flat[14, 4] = -100


def gen(name, seed, pc, ncb, hidden, K, B, reduction, lead=None, pad=pad_whole_frames):
    torch.manual_seed(seed)
    m = refq.JointCodebookLoss(predictor_channels=pc, num_codebooks=ncb, hidden_channels=hidden, codebook_size=K,
                               reduction=reduction, checkpoint=False)
    with torch.no_grad():
        m.linear2_bias.normal_(std=0.1)      # zeros at init: make the bias path visible
    shape = (B,) if lead is None else lead
    pred = torch.randn(*shape, pc, requires_grad=True)
    idx = torch.randint(0, K, (*shape, ncb))
    flat = idx.reshape(-1, ncb)
    pad(flat)
    loss = m(pred, idx)
    loss.backward()
    out = dict(pc=pc, ncb=ncb, hidden=hidden, K=K, reduction=reduction, predictor=pred.detach().numpy(),
               indexes=idx.numpy(), loss=float(loss), grad_predictor=pred.grad.numpy())
    for k, v in m.state_dict().items():
        out["state." + k] = v.numpy()
    for k, p in m.named_parameters():
        out["grad." + k] = p.grad.numpy()
    np.savez_compressed(os.path.join(HERE, f"jcl_{name}.npz"), **out)
    print(name, "loss", float(loss))


CASES = {
    "small_k16": dict(seed=3, pc=48, ncb=4, hidden=32, K=16, B=70, reduction="sum"),
    "k256_n4": dict(seed=4, pc=32, ncb=4, hidden=48, K=256, B=96, reduction="sum", lead=(4, 24)),
    "mean_k64": dict(seed=5, pc=40, ncb=2, hidden=64, K=64, B=50, reduction="mean"),
    "partial_k32": dict(seed=6, pc=24, ncb=5, hidden=40, K=32, B=60, reduction="sum", pad=pad_partial),
}

if __name__ == "__main__":
    for name_ in sys.argv[1:] or CASES:
        gen(name_, **CASES[name_])
