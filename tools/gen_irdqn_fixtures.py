"""Generate tests/golden/irdqn_*.npz from the reference's algorithms/irdqn.py (build container only; imports the
reference through tools/ref_import.py and the recording env wrapper of tools/gen_fixtures.py).

  python tools/gen_irdqn_fixtures.py

Per case (loss 'huber' / 'mse'): 2 agents, hidden 100, the reference CombinatorialEnv with 4 channels and short
deadlines, episode_length 10, history_len 5, gamma 0.4, lr 1e-4, minibatch 8 (the drivers' iRDQN block scaled down).
Recorded (numeric arrays and a params_json of constructor kwargs, nothing else):
irdqn_common.npz (one seed serves both losses):
  weights/agent{i}/network/...            the initial state_dicts (the target network is a copy, irdqn.py:129)
  test/...       iRDQN.test(4) at the initial weights: env draws, greedy actions, the returned tuple, per decision
                 the Q-values' top-2 gap
  buffer/...     the transitions of 6 training episodes (exploring: replay_start_size beyond them) through a replay
                 buffer of 40: obs rows per episode (reset obs + every next obs), actions, rewards, done
irdqn_{huber,mse}.npz:
  upd/...        K = 3 updates as iRDQN.train runs them (irdqn.py:285-300: ReplayBuffer.sample_chunk, the per-agent
                 slices, DQN.train_step) with the networks cast to float64, so a float64 re-implementation can be
                 pinned to them: chunk starts, per update and agent the loss and delta; every .grad of the first
                 update of agent 0 in full, of the others as (sum, abs-sum, abs-max) -- each file stays under 1 MiB
  weights_after/agent{i}/...              the network weights after the K updates (float32)
The generator asserts that every recorded greedy decision has a top-2 gap >= 1e-3 and that every huber minibatch
holds samples with |delta| < 1 and with |delta| > 1, and tries the next seed otherwise."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_fixtures import OUT, RecordingEnv, _jsonable, _put, _sd_np  # noqa: E402
from ref_import import ref_module  # noqa: E402

K, N_TEST, N_TRAIN, BUFFER = 3, 4, 6, 40
ENV = dict(n_agents=2, n_channels=4, deadlines=np.array([3, 4]), lbdas=np.array([0.8, 0.8]), episode_length=10,
           traffic_model="aperiodic", homogeneous_size=True, channel_switch=np.array([0.3, 0.5, 0.7, 0.4]))
LEARNER = dict(history_len=5, replay_start_size=10 ** 6, replay_buffer_size=BUFFER, gamma=0.4,
               update_target_frequency=10 ** 6, minibatch_size=8, learning_rate=1e-4)


def generate(loss, seed):
    import torch
    irdqn = ref_module("algorithms.irdqn")
    env = ref_module("envs.combinatorial_env").CombinatorialEnv(**ENV)
    torch.manual_seed(seed)
    np.random.seed(seed + 1)
    import random
    random.seed(seed + 2)
    lr = irdqn.iRDQN(env, loss=loss, **LEARNER)
    out = {"loss": loss, "seed": seed, "K": K,
           "params_json": json.dumps({"env": {k: _jsonable(v) for k, v in ENV.items()}, "learner": LEARNER})}
    per = {"loss": loss, "seed": seed, "K": K}
    for i, a in enumerate(lr.agents):        # the target is a copy of the network at construction (irdqn.py:129)
        _put(out, f"weights/agent{i}/network", _sd_np(a.network))
        assert all(np.array_equal(v, _sd_np(a.network)[k]) for k, v in _sd_np(a.target_network).items())

    # ---- test(): greedy actions on recorded draws, with every decision's top-2 gap
    gaps = []
    hooks = [a.network.register_forward_hook(
        lambda m, i, o: gaps.append(float(np.diff(np.sort(o.detach().numpy().ravel())[-2:])[0]))) for a in lr.agents]
    rec = RecordingEnv(env)
    lr.env = rec
    res = lr.test(N_TEST)
    for h in hooks:
        h.remove()
    if min(gaps) < 1e-3:
        return None
    for k, v in rec.rec.items():
        out[f"test/draws/{k}"] = np.array(v)
    out["test/result"] = np.array([float(x) for x in res], dtype=np.float64)
    out["test/gaps"] = np.array(gaps)

    # ---- training episodes into the reference's replay buffer (every action explores: not training-ready)
    lr.env = env
    # (the loop of iRDQN.train, irdqn.py:230-268, without its test(50) at episode 0)
    obs_rows, acts, rews, dones = [], [], [], []
    for ep in range(N_TRAIN):
        state, _ = env.reset()
        state = torch.tensor(np.stack(state), dtype=torch.float)
        obs_rows.append(state.numpy().copy())
        done = False
        while not done:
            actions = np.array([a.act(None, is_training_ready=False) for a in lr.agents])
            binary = np.zeros((env.n_agents, env.n_channels))
            binary[np.arange(env.n_agents), actions] = 1
            state_next, _, rewards, done, _ = env.step(binary)
            state_next = torch.tensor(np.stack(state_next), dtype=torch.float)
            lr.replay_buffer.add((state, actions, rewards, state_next, done))
            obs_rows.append(state_next.numpy().copy())
            acts.append(actions)
            rews.append(np.asarray(rewards, dtype=np.float64))
            dones.append(bool(done))
            state = state_next
    out["buffer/obs"] = np.array(obs_rows, dtype=np.float32).reshape(N_TRAIN, ENV["episode_length"] + 1,
                                                                      env.n_agents, -1)
    out["buffer/actions"] = np.array(acts, dtype=np.int64)
    out["buffer/rewards"] = np.array(rews)
    out["buffer/done"] = np.array(dones)
    assert len(lr.replay_buffer) == BUFFER

    # ---- K updates in float64 (the train loop's body, irdqn.py:287-298)
    for a in lr.agents:
        a.network.double()
        a.target_network.double()
    L, B = LEARNER["history_len"], LEARNER["minibatch_size"]
    for u in range(K):
        st = np.random.get_state()
        tr = lr.replay_buffer.sample_chunk(B, L)
        after = np.random.get_state()
        np.random.set_state(st)
        per[f"upd/{u}/starts"] = np.random.randint(0, len(lr.replay_buffer) - L, B)
        np.random.set_state(after)
        tr = [t.double() if t.is_floating_point() else t for t in tr]
        for i, a in enumerate(lr.agents):
            t_i = (tr[0][:, :, i, :], tr[1][:, -1, i].unsqueeze(1), tr[2][:, -1, i].unsqueeze(1), tr[3][:, :, i, :],
                   tr[4][:, -1, :])
            with torch.no_grad():
                qt = a.target_network(t_i[3]).max(1, True)[0]
                delta = (a.network(t_i[0]).gather(1, t_i[1]) - (t_i[2] + (1 - t_i[4]) * a.gamma * qt)).numpy().ravel()
            if loss == "huber" and not ((np.abs(delta) < 1).any() and (np.abs(delta) > 1).any()):
                return None
            per[f"upd/{u}/agent{i}/delta"] = delta
            per[f"upd/{u}/agent{i}/loss"] = np.float64(a.train_step(t_i))
            for n, prm in a.network.named_parameters():      # .grad as left by train_step's backward
                g = prm.grad.detach().numpy().copy()
                if u == 0 and i == 0:                        # in full (float64); the others as checksums (file size)
                    per[f"upd/{u}/agent{i}/grad/{n}"] = g
                per[f"upd/{u}/agent{i}/gradsum/{n}"] = np.array([g.sum(), np.abs(g).sum(), np.abs(g).max()])
    for i, a in enumerate(lr.agents):
        _put(per, f"weights_after/agent{i}", {k: v.astype(np.float32) for k, v in _sd_np(a.network).items()})
    return out, per


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    # one seed for both losses: the weights, the test() trace and the buffer are shared (irdqn_common.npz)
    for seed in range(100, 140):
        res = [generate(loss, seed) for loss in ("huber", "mse")]
        if any(r is None for r in res):
            continue
        (common, huber), (common2, mse) = res
        assert all(np.array_equal(common[k], common2[k]) for k in common if k not in ("loss", "params_json"))
        common.pop("loss")
        for name, out in (("common", common), ("huber", huber), ("mse", mse)):
            path = os.path.join(OUT, f"irdqn_{name}.npz")
            np.savez_compressed(path, **out)
            assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
            print(f"irdqn_{name}: seed {seed}, {os.path.getsize(path)} bytes")
        print(f"test result {common['test/result']}, min gap {common['test/gaps'].min():.3g}, losses "
              f"{[[float(o[f'upd/{u}/agent0/loss']) for u in range(K)] for o in (huber, mse)]}")
        break
    else:
        raise SystemExit("no seed satisfied the conditions")
