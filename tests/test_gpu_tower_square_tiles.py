"""The square-tile tower (k_tower_sq: 5×5 boards, 64 filters, full batches; one board square per MFMA row tile, off-board taps
skipped) must return the BITS of the plain-image tower k_tower (TG_NO_HALO_TOWER=1).  The launchers' switches are read once
per process, so every variant runs in its own process; each process hashes policy + eval of several batch sizes, ragged last
workgroups included."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("TG_NO_HALO_TOWER", "TG_NO_FRAG_OUT", "TG_NO_CONST_BIAS", "TG_PRECISION", "TG_NO_SPLIT_TOWER")
BATCHES = (2049, 4093, 4096, 4096 + 13)

DIGESTS = r"""
import hashlib, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
import numpy as np
import posgen, tak_amd, torch_ref
from oracle import oracle as orc
orc.lib()
batches = {batches!r}
net = torch_ref.make_net(5, {blocks}, 64, "fc5", seed=7, randomize_bn={bn!r})
e = tak_amd.Engine(5, res_blocks={blocks}, filters=64, evaluator=tak_amd.EVAL_RESNET, max_batch=max(batches))
e.load_state_dict(torch_ref.abi_tensors(net))
sts = posgen.distinct_positions(orc, 5, max(batches), seed=31, max_plies=60)
out = []
for b in batches:
    p, v = e.policy_eval(sts[:b])
    assert np.isfinite(p).all() and np.isfinite(v).all()
    out.append(hashlib.sha256(np.ascontiguousarray(p).tobytes() + np.ascontiguousarray(v).tobytes()).hexdigest())
print(" ".join(out))
"""


def _digests(blocks, bn, batches, **env):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update(env)
    code = DIGESTS.format(root=ROOT, batches=tuple(batches), blocks=blocks, bn=bn)
    out = subprocess.run([sys.executable, "-c", code], env=e, check=True, capture_output=True, text=True, timeout=600)
    return out.stdout.strip().splitlines()[-1].split()


@pytest.mark.gpu
def test_square_tiles_return_the_bits_of_the_plain_tower_at_every_full_batch():
    """randomised BatchNorm fold, the constant-planes bias entry (the benchmarked one), 2049 … 4109 positions"""
    base = _digests(6, True, BATCHES)
    assert len(base) == len(BATCHES) and len(set(base)) == len(BATCHES)
    assert _digests(6, True, BATCHES, TG_NO_HALO_TOWER="1") == base


@pytest.mark.gpu
def test_square_tiles_planes_entry_and_row_major_output():
    """layer 0 over every input plane (TG_NO_CONST_BIAS: the CH0 = 5 instantiation) and the row-major output (TG_NO_FRAG_OUT)"""
    batches = (2049, 4093)
    dense = _digests(6, True, batches, TG_NO_CONST_BIAS="1")
    assert _digests(6, True, batches, TG_NO_CONST_BIAS="1", TG_NO_HALO_TOWER="1") == dense
    base = _digests(6, True, batches)
    assert _digests(6, True, batches, TG_NO_FRAG_OUT="1") == base
    assert _digests(6, True, batches, TG_NO_FRAG_OUT="1", TG_NO_HALO_TOWER="1") == base


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [0, 1])
def test_square_tiles_on_networks_with_few_blocks(blocks):
    """no residual block (layer 0 is the tower's output) and a single one (the layer loop ends on its first conv2)"""
    batches = (2049, 4093)
    base = _digests(blocks, True, batches)
    assert _digests(blocks, True, batches, TG_NO_HALO_TOWER="1") == base
