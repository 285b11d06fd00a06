"""Generate tests/golden/loss_train_golden.npz (authoring container only: needs the reference checkout).

    python tests/golden/make_loss_train_golden.py

Recorded: the REAL reference's forwardDirection / reverseDirection (oracle/ref_loader.py) in train(), fp32 on the CPU, composed as
model_building.py:141-157 composes them, with synth.make_synergy_state(loss_cases.SEED_SYN) -- 'plain' -- and with
loss_train_cases.edge_state of it -- 'edge': an eighth of every BatchNorm's gamma negated, a sixteenth set to 0 -- on the first B of
loss_grad_cases.candidate_inputs() for B in loss_train_cases.BATCHES.  Per case <state>|B<B>|<field>:
  * the five weighted losses, S2 [B,62], the refined landmarks [B,3,68];
  * mean / var: every BatchNorm's batch mean and BIASED variance of the first call, taken by forward hooks from the module's input;
  * run1_* / run3_*: running_mean / running_var after one and after three calls on the same batch (momentum 0.1).
The per-channel vectors keep loss_train_cases.recorded_channels() of the 3649 channels.  Every value is computed a second time in
float64 and must agree within 1e-5 (losses relative, S2 / landmarks relative to the max of the tensor, statistics relative to the max
of their BatchNorm's tensor).  Data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))

import loss_cases as lc                   # noqa: E402
import loss_train_cases as lt             # noqa: E402
from oracle import ref_loader             # noqa: E402
from synergynet_amd import synth          # noqa: E402


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    g = dict(np.load(os.path.join(HERE, 'reference_outputs.npz'), allow_pickle=False))
    pack = synth.make_3dmm(int(g['seeds'][1]))
    ref = ref_loader.load_reference(pack)
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    base = synth.make_synergy_state(lc.SEED_SYN)
    model = ref.SynergyNet()
    mods = list(zip((model.forwardDirection, model.reverseDirection), synth.SYNERGY_PREFIXES))
    bns = [(name, dict(mod.named_modules())[name[len(prefix):]]) for name, _ in lt.bn_order() for mod, prefix in mods if name.startswith(prefix)]
    assert len(bns) == len(lt.bn_order()) and all(isinstance(m, torch.nn.BatchNorm1d) and m.momentum == lt.MOMENTUM and m.eps == lt.EPS for _, m in bns)

    def load(sd, dt):
        model.float()
        for mod, prefix in mods:
            own = mod.state_dict()
            mod.load_state_dict({k: t(np.asarray(sd[prefix + k])) if prefix + k in sd else v for k, v in own.items()})
        model.eval()                                   # the 3DMM part has no mode; the two MLPs go to train() as main_train.py:113 puts them
        model.forwardDirection.train()
        model.reverseDirection.train()
        if dt == torch.float64:
            model.double()

    def call(B, dt, seen):
        param, pool, target = lt.inputs(B)
        a, avgpool, gt = t(param, dt), t(pool, dt), t(target, dt)
        hooks = [m.register_forward_hook(lambda mod, inp, out, name=name: seen.append((name, inp[0].detach()))) for name, m in bns]
        with torch.no_grad():
            loss = {}
            vertex_lmk = model.reconstruct_vertex_62(a, dense=False)
            vertex_GT_lmk = model.reconstruct_vertex_62(gt, dense=False)
            loss['loss_LMK_f0'] = 0.05 * model.LMKLoss_3D(vertex_lmk, vertex_GT_lmk, kp=True)
            loss['loss_Param_In'] = 0.02 * model.ParamLoss(a, gt)
            vertex_lmk = vertex_lmk + 0.05 * model.forwardDirection(vertex_lmk, avgpool, a[:, 12:52], a[:, 52:62])
            loss['loss_LMK_pointNet'] = 0.05 * model.LMKLoss_3D(vertex_lmk, vertex_GT_lmk, kp=True)
            s2 = model.reverseDirection(vertex_lmk)
            loss['loss_Param_S2'] = 0.02 * model.ParamLoss(s2, gt, mode='only_3dmm')
            loss['loss_Param_S1S2'] = 0.001 * model.ParamLoss(s2, a, mode='only_3dmm')
        for h in hooks:
            h.remove()
        out = {k: loss[k].numpy() for k in lc.LOSS_NAMES}
        out.update(S2=s2.numpy(), Lr=vertex_lmk.numpy())
        return out

    def running():
        return (torch.cat([m.running_mean for _, m in bns]).numpy().copy(), torch.cat([m.running_var for _, m in bns]).numpy().copy())

    def case(sd, B, dt):
        load(sd, dt)
        out = None
        for c in range(1, lt.CALLS + 1):
            seen = []
            r = call(B, dt, seen)
            if c == 1:
                out = r
                assert [n for n, _ in seen] == [n for n, _ in lt.bn_order()]
                dims = lambda x: (0, 2) if x.dim() == 3 else (0,)
                out['mean'] = torch.cat([x.mean(dims(x)) for _, x in seen]).numpy()
                out['var'] = torch.cat([x.var(dims(x), unbiased=False) for _, x in seen]).numpy()
            if c in (1, lt.CALLS):
                out[f'run{c}_mean'], out[f'run{c}_var'] = running()
        return out

    keep = lt.recorded_channels()
    out = dict(torch_version=np.array(torch.__version__), graph_seed=np.array(lc.SEED_SYN), channels=keep.astype(np.int32))
    worst = {}
    for state in lt.STATES:
        sd = lt.state_of(base, state)
        for B in lt.BATCHES:
            r32, r64 = case(sd, B, torch.float32), case(sd, B, torch.float64)
            for f in lt.RECORDED_FIELDS:
                e = lt.rel(r32[f], r64[f], f)
                fam = 'losses' if f in lc.LOSS_NAMES else f
                worst[fam] = max(worst.get(fam, 0.0), e)
                assert e <= lt.CPU_BAR, (state, B, f, e)
                v = np.asarray(r32[f], dtype=np.float32)
                out[lt.case_key(state, B, f)] = v[keep] if f in lt.PER_CHANNEL else v
    print('worst fp32 / fp64 disagreement per field:', {k: '%.2g' % v for k, v in worst.items()}, 'bar', lt.CPU_BAR)
    np.savez_compressed(lt.GOLDEN, **out)
    print('wrote', lt.GOLDEN, os.path.getsize(lt.GOLDEN), 'bytes')
    assert os.path.getsize(lt.GOLDEN) < 512 << 10


if __name__ == '__main__':
    main()
