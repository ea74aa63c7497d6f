"""iRDQN — drop-in for /root/reference/algorithms/irdqn.py (independent recurrent DQN: one GRU Q-network and one
target network per agent on its own observation history; the value-based baseline D2D-PPO is compared against).

Same module-level API (Transition, ReplayBuffer, init_weights, RNN, DQN, iRDQN), constructor signatures,
train(n_episodes, early_stopping=True) / test(n_episodes, verbose=False) and return values.  The work runs
agent-batched on the MI355X (csrc/rdqn_kernels.hip through d2dhip/rdqn.py):
  * acting: ONE d2d_rdqn_q launch per slot gives every agent's epsilon-greedy action in every env of the batch
    (the reference: N batch-1 GRU forwards per slot, irdqn.py:244-253), then the env-step kernel;
  * replay: a device ring per env timeline, episode_length + 1 obs rows per episode (the reset obs and every next
    obs), so transition t's state is row t of its episode and its successor state row t + 1 -- s' is not stored twice;
    fp32 rows by default, or (replay_record=True / D2D_RDQN_RECORD=1) the env kernel's compact obs record, 32 bytes
    per agent row instead of 4 * obs_dim, with bit-identical results;
  * acting state: while a slot's window is still an episode prefix (t + 1 <= history_len) its hidden state is the
    previous slot's plus one GRU step, so the launch carries it (d2dhip.rdqn.CarryState) instead of recomputing the
    window, bit for bit the same actions (carry_state / D2D_RDQN_CARRY=0 turns it off);
  * update: one d2d_rdqn_q launch on the target parameters (max_a Q'(s')), one d2d_rdqn_grad launch (TD loss and
    BPTT gradients of all N agents, written into .grad) and one Adam step over the agent-stacked parameters (the
    reference: N x (two GRU forwards, one backward, one Adam step), irdqn.py:290-300).

Reference semantics kept (each exactly the reference's at n_envs = 1): see episode_plan / wave_events below and
DESIGN.md §4.9.  Not implemented: a callable `loss` (NotImplementedError); shapes outside the kernels' envelope
(hidden <= 128, obs + 1 <= 64, n_channels <= 16, history_len <= 256) raise NotImplementedError.
"""
import functools
import math
import os
import random
from collections import deque, namedtuple

import numpy as np
import torch
import torch.nn as nn

from ._core import gru_window, init_weights  # noqa: F401
from ._learner import BatchedLearnerBase

Transition = namedtuple('Transition', ('state', 'action', 'reward', 'state_next', 'done'))

HORIZON_EPS = 1000   # DQN.update_epsilon's default horizon (irdqn.py:159), never overridden by the reference
TEST_EVERY = 100     # iRDQN.train tests and prints every 100 episodes (irdqn.py:274)
TEST_EPISODES = 50


class ReplayBuffer:
    """The reference's host replay buffer (irdqn.py:15-48), kept for direct callers: a deque of
    (state, action, reward, state_next, done) whose sample_chunk draws `batch_size` chunks of `chunk_size`
    consecutive transitions, starts uniform in [0, len - chunk_size) from numpy's global RNG."""

    def __init__(self, buffer_limit, device):
        self.buffer = deque(maxlen=buffer_limit)
        self.device = device
        self.buffer_limit = buffer_limit

    def add(self, transition):
        self.buffer.append(transition)

    def sample_chunk(self, batch_size, chunk_size):
        starts = np.random.randint(0, len(self.buffer) - chunk_size, batch_size)
        rows = [self.buffer[j] for s in starts for j in range(s, s + chunk_size)]
        s, a, r, sn, d = zip(*rows)
        n_agents, obs_size = s[0].shape[0], s[0].shape[1]
        shape = (batch_size, chunk_size, n_agents)
        return (torch.stack(s).view(*shape, obs_size).to(self.device),
                torch.tensor(np.stack(a), dtype=torch.long).view(shape).to(self.device),
                torch.tensor(np.stack(r), dtype=torch.float).view(shape).to(self.device),
                torch.stack(sn).view(*shape, obs_size).to(self.device),
                torch.tensor(d, dtype=torch.float).view(batch_size, chunk_size, 1).to(self.device))

    def reset(self):
        self.buffer = deque(maxlen=self.buffer_limit)

    def __len__(self):
        return len(self.buffer)


class RNN(torch.nn.Module):
    """irdqn.py:58-86: GRU over the window from h0 = 0 -> Linear -> ReLU -> Linear -> ReLU -> Linear (orthogonal
    gain 3, zero bias), no output activation.  forward takes (L, in) or (B, L, in) like the reference."""

    def __init__(self, n_inputs, n_outputs, hidden_size=100, **kwargs):
        super().__init__()
        self.hidden_size = hidden_size
        self.lstm = nn.GRU(n_inputs, hidden_size, 1)
        self.layers = nn.Sequential(nn.Linear(hidden_size, hidden_size), nn.ReLU(),
                                    nn.Linear(hidden_size, hidden_size), nn.ReLU(),
                                    nn.Linear(hidden_size, n_outputs))
        self.layers.apply(lambda x: init_weights(x, 3))

    def init_hidden(self, batch_size):
        return (torch.zeros(1, batch_size, self.hidden_size), torch.zeros(1, batch_size, self.hidden_size))

    def forward(self, obs):
        if len(obs.shape) == 2:
            obs = obs.unsqueeze(0)
        w = self.lstm
        h = gru_window(obs.unsqueeze(0), w.weight_ih_l0.unsqueeze(0), w.weight_hh_l0.unsqueeze(0),
                       w.bias_ih_l0.unsqueeze(0), w.bias_hh_l0.unsqueeze(0))[0]
        return self.layers(h)


class StackedQNets:
    """Agent-stacked storage of N irdqn RNN modules (the sibling of _core.StackedNets for the three-layer head):
    `params` name -> nn.Parameter [N, ...] in d2dhip.rdqn.NAMES order; each module's parameters are views."""

    def __init__(self, modules, in_dims, device):
        self.N = len(modules)
        self.in_dims = [int(d) for d in in_dims]
        self.F = max(self.in_dims)
        m0 = modules[0]
        self.H, self.A = m0.hidden_size, m0.layers[4].out_features
        H, A, F = self.H, self.A, self.F
        shapes = {"w_ih": (3 * H, F), "w_hh": (3 * H, H), "b_ih": (3 * H,), "b_hh": (3 * H,), "w1": (H, H), "b1": (H,),
                  "w2": (H, H), "b2": (H,), "w3": (A, H), "b3": (A,)}
        self.params = {}
        with torch.no_grad():
            for name, shp in shapes.items():
                t = torch.zeros((self.N,) + shp, dtype=torch.float32)
                for k, m in enumerate(modules):
                    src = self._srcs(m)[name].detach().to("cpu", torch.float32)
                    if name == "w_ih":
                        t[k, :, : self.in_dims[k]] = src
                    else:
                        t[k] = src
                self.params[name] = nn.Parameter(t.to(torch.device(device)))
        for k, m in enumerate(modules):
            self._bind(m, k)

    @staticmethod
    def _srcs(m):
        return {"w_ih": m.lstm.weight_ih_l0, "w_hh": m.lstm.weight_hh_l0, "b_ih": m.lstm.bias_ih_l0,
                "b_hh": m.lstm.bias_hh_l0, "w1": m.layers[0].weight, "b1": m.layers[0].bias,
                "w2": m.layers[2].weight, "b2": m.layers[2].bias, "w3": m.layers[4].weight, "b3": m.layers[4].bias}

    def _bind(self, m, k):
        p = {n: t.data[k] for n, t in self.params.items()}
        m.to(self.params["b1"].device)
        m.lstm.weight_ih_l0 = nn.Parameter(p["w_ih"][:, : self.in_dims[k]])
        m.lstm.weight_hh_l0 = nn.Parameter(p["w_hh"])
        m.lstm.bias_ih_l0 = nn.Parameter(p["b_ih"])
        m.lstm.bias_hh_l0 = nn.Parameter(p["b_hh"])
        for i, (wn, bn) in ((0, ("w1", "b1")), (2, ("w2", "b2")), (4, ("w3", "b3"))):
            m.layers[i].weight = nn.Parameter(p[wn])
            m.layers[i].bias = nn.Parameter(p[bn])

    def parameters(self):
        return list(self.params.values())

    def data(self):
        return {k: v.data for k, v in self.params.items()}

    def copy_from(self, other):
        with torch.no_grad():
            for k, v in self.params.items():
                v.copy_(other.params[k])


def epsilon_at(timestep, initial, final, horizon_eps=HORIZON_EPS):
    """DQN.update_epsilon (irdqn.py:159-161): linear from initial to final over horizon_eps episodes."""
    return max(initial - (initial - final) * (timestep / horizon_eps), final)


def episode_plan(ep, replay_start_size, update_frequency, update_target_frequency, initial, final):
    """What the reference's train loop does in episode `ep` (irdqn.py:230-300), as host data:
    ready      is_training_ready = ep >= replay_start_size (episodes, not transitions);
    eps_first  the epsilon of slot 0: update_epsilon(ep) follows act (irdqn.py:247-253), so slot 0 still sees
               epsilon(ep - 1).  Episode 0 starts at `initial`: the reference has no epsilon attribute yet and would
               raise AttributeError there when replay_start_size == 0; otherwise slot 0 of episode 0 explores anyway;
    eps        the epsilon of every later slot, epsilon(ep);
    test       ep % 100 == 0 (test(50), print, early stop when the score is 1) -- before the update;
    update     ready and ep % update_frequency == 0: one minibatch update of every agent;
    sync       update and ep % update_target_frequency == 0: target <- network, after the update."""
    ready = ep >= replay_start_size
    update = ready and ep % update_frequency == 0
    return dict(ep=ep, ready=ready, eps_first=epsilon_at(ep - 1, initial, final) if ep > 0 else initial,
                eps=epsilon_at(ep, initial, final), test=ep % TEST_EVERY == 0, update=update,
                sync=update and ep % update_target_frequency == 0)


def wave_events(ep0, n_envs, n_episodes, **kw):
    """The ordered end-of-episode events of the wave that runs episodes ep0 .. ep0 + n_envs - 1 side by side (those
    below n_episodes): ('test' | 'update' | 'sync', ep), what the reference would have run after each of them."""
    ev = []
    for ep in range(ep0, min(ep0 + n_envs, n_episodes)):
        p = episode_plan(ep, **kw)
        ev += [(name, ep) for name in ("test", "update", "sync") if p[name]]
    return ev


class DQN:
    """Per-agent object (irdqn.py:88-166).  Its networks are views into the learner's agent-stacked parameters;
    act / predict / train_step keep the reference's single-agent semantics for direct callers."""

    def __init__(self, env, replay_start_size=50000, replay_buffer_size=1000000, gamma=0.99,
                 update_target_frequency=10000, minibatch_size=32, learning_rate=1e-3, update_frequency=1,
                 initial_exploration_rate=1, final_exploration_rate=0.1, adam_epsilon=1e-8, loss='huber',
                 agent_index=0, device=None):
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.replay_start_size = replay_start_size
        self.replay_buffer_size = replay_buffer_size
        self.gamma = gamma
        self.update_target_frequency = update_target_frequency
        self.minibatch_size = minibatch_size
        self.learning_rate = learning_rate
        self.update_frequency = update_frequency
        self.initial_exploration_rate = initial_exploration_rate
        self.final_exploration_rate = final_exploration_rate
        self.adam_epsilon = adam_epsilon
        if callable(loss):
            raise NotImplementedError("iRDQN on the HIP kernels implements loss 'huber' and 'mse', not a callable")
        self.loss = {'huber': torch.nn.functional.smooth_l1_loss, 'mse': torch.nn.functional.mse_loss}[loss]
        self.env = env
        state_size = self.env.observation_space[agent_index].shape[0]
        action_size = self.env.action_space[agent_index].n
        self.network = RNN(state_size, action_size)
        self.target_network = RNN(state_size, action_size)
        self.target_network.load_state_dict(self.network.state_dict())
        self.optimizer = None
        self.epsilon = initial_exploration_rate

    def train_step(self, transitions):
        if self.optimizer is None:
            self.optimizer = torch.optim.Adam(self.network.parameters(), lr=self.learning_rate, eps=self.adam_epsilon)
        states, actions, rewards, states_next, dones = transitions
        with torch.no_grad():
            q_value_target = self.target_network(states_next).max(1, True)[0]
        td_target = rewards + (1 - dones) * self.gamma * q_value_target
        q_value = self.network(states).gather(1, actions)
        loss = self.loss(q_value, td_target, reduction='mean')
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        return loss.item()

    def act(self, state, is_training_ready=True):
        if is_training_ready and random.uniform(0, 1) >= self.epsilon:
            return self.predict(state)
        return np.random.randint(0, 2)  # irdqn.py:154: explore actions come from {0, 1}

    def update_epsilon(self, timestep, horizon_eps=HORIZON_EPS):
        self.epsilon = epsilon_at(timestep, self.initial_exploration_rate, self.final_exploration_rate, horizon_eps)

    @torch.no_grad()
    def predict(self, state):
        return self.network(state).argmax().item()


def _fused_optimizer_kwarg(init):
    """iRDQN(..., fused_optimizer=True / False) without another named parameter: the constructor's signature -- the
    reference's order, then replay_record -- is pinned (tests/test_irdqn_record_cpu.py), so the keyword is taken
    off here, before the constructor proper runs, and overrides the class default (D2D_FUSED_OPTIM)."""
    @functools.wraps(init)
    def wrapped(self, *args, fused_optimizer=None, **kw):
        if fused_optimizer is not None:
            self.fused_optimizer = bool(fused_optimizer)
        return init(self, *args, **kw)
    return wrapped


class iRDQN(BatchedLearnerBase):
    # the replay / test rings as the compact obs record instead of fp32 rows (the same results, a quarter of the bytes)
    replay_record = os.environ.get("D2D_RDQN_RECORD", "0") == "1"
    # acting slots carry their hidden state while the window is an episode prefix (the same results, fewer GRU steps)
    carry_state = os.environ.get("D2D_RDQN_CARRY", "1") != "0"

    @_fused_optimizer_kwarg
    def __init__(self, env, history_len=5, replay_start_size=50000, replay_buffer_size=1000000, gamma=0.99,
                 update_target_frequency=10000, minibatch_size=32, learning_rate=1e-3, update_frequency=1,
                 initial_exploration_rate=1, final_exploration_rate=0.1, adam_epsilon=1e-8, loss='huber',
                 early_stopping=True, *, replay_record=None):
        """The reference's arguments, then two keyword-only switches: replay_record (the replay ring as the compact obs
        record) and fused_optimizer (True: the Adam step as one d2d_adam_step call, d2dhip.optim.StackedAdam; None: the
        class default, D2D_FUSED_OPTIM).  fused_optimizer is accepted by the _fused_optimizer_kwarg wrapper and does
        not show in this signature or in help()."""
        self.device = self._resolve_device(None)
        if self.device.type != "cuda":
            import d2dhip
            d2dhip.require_gpu()
        if callable(loss):
            raise NotImplementedError("iRDQN on the HIP kernels implements loss 'huber' and 'mse', not a callable")
        self.history_len = history_len
        if replay_record is not None:
            self.replay_record = bool(replay_record)
        self._carries = {}        # (id(batch), role) -> rdqn.CarryState
        self.replay_start_size = replay_start_size
        self.replay_buffer_size = replay_buffer_size
        self.replay_buffer = ReplayBuffer(self.replay_buffer_size, self.device)  # reference attribute; unused here
        self.gamma = gamma
        self.update_target_frequency = update_target_frequency
        self.minibatch_size = minibatch_size
        self.learning_rate = learning_rate
        self.update_frequency = update_frequency
        self.initial_exploration_rate = initial_exploration_rate
        self.final_exploration_rate = final_exploration_rate
        self.adam_epsilon = adam_epsilon
        self.early_stopping = early_stopping
        self.loss_name = loss
        self.loss = {'huber': torch.nn.functional.smooth_l1_loss, 'mse': torch.nn.functional.mse_loss}[loss]
        self.env = env
        self.n_agents = env.n_agents
        kw = dict(replay_start_size=replay_start_size, replay_buffer_size=replay_buffer_size, gamma=gamma,
                  update_target_frequency=update_target_frequency, minibatch_size=minibatch_size,
                  learning_rate=learning_rate, update_frequency=update_frequency,
                  initial_exploration_rate=initial_exploration_rate, final_exploration_rate=final_exploration_rate,
                  adam_epsilon=adam_epsilon, loss=loss)
        self.agents = [DQN(env, agent_index=k, device=self.device, **kw) for k in range(env.n_agents)]
        in_dims = [env.observation_space[k].shape[0] for k in range(env.n_agents)]
        self.network = StackedQNets([a.network for a in self.agents], in_dims, self.device)
        self.target_network = StackedQNets([a.target_network for a in self.agents], in_dims, self.device)
        from d2dhip import rdqn
        if env.kind != "comb":
            raise NotImplementedError("iRDQN acts through one-hot channel masks: the combinatorial env only "
                                      "(the reference's iRDQN.train builds action_binary over env.n_channels)")
        if self.network.A != env.n_channels:
            raise NotImplementedError("iRDQN needs one action per channel")
        rdqn.check_envelope(self.network.F, self.network.H, self.network.A, history_len)
        if self.fused_optimizer:
            self.optimizer = self._stacked_adam(self.network.parameters(), self.n_agents, learning_rate,
                                                eps=adam_epsilon)
        else:
            self.optimizer = torch.optim.Adam(self.network.parameters(), lr=learning_rate, eps=adam_epsilon)
        self.losses = []          # per update: loss [N] (device tensors)
        self.n_updates = self.n_syncs = 0

    # ------------------------------------------------------------ schedule
    def _plan_kw(self):
        return dict(replay_start_size=self.replay_start_size, update_frequency=self.update_frequency,
                    update_target_frequency=self.update_target_frequency, initial=self.initial_exploration_rate,
                    final=self.final_exploration_rate)

    # --------------------------------------------------------------- replay
    def _alloc_ring(self, b, n_waves):
        """Per env timeline: whole episodes of T + 1 obs rows, actions / rewards per transition.  Capacity
        floor(replay_buffer_size / E) transitions per env (the deque's maxlen, split over the envs), bounded by
        what this train() call can produce; one more episode of rows than the capacity needs, so the transitions
        still inside the capacity are never the ones being overwritten."""
        s, E, T, dev = b.spec, b.E, self.env.episode_length, self.device
        cap = max(1, self.replay_buffer_size // E)
        n_ep = min(n_waves, -(-cap // T) + 1)
        self._cap = min(cap, n_waves * T)
        self._ring_ep = n_ep
        self._ring = self._obs_ring(b, n_ep * (T + 1))
        self._act_ring = torch.zeros((n_ep * T, E, s.N), dtype=b.action_buffer().dtype, device=dev)
        self._rew_ring = torch.zeros((n_ep * T, E), dtype=torch.int32, device=dev)
        self._added = 0           # transitions written per env so far

    def _obs_ring(self, b, rows):
        """A zeroed obs ring [rows][E][N][F]: fp32 rows, or the env batch's compact record (replay_record)."""
        if self.replay_record:
            return b.record_buffer((rows,))
        s = b.spec
        return torch.zeros((rows, b.E, s.N, s.F), dtype=torch.float32, device=self.device)

    def _carry(self, b, role):
        """The CarryState of (batch, role), or None with carry_state off."""
        if not self.carry_state:
            return None
        from d2dhip import rdqn
        key = (id(b), role)
        carries = self.__dict__.setdefault("_carries", {})
        if key not in carries:
            carries[key] = rdqn.CarryState()
        return carries[key]

    def _sample_chunks(self, n_envs, length, batch_size, chunk_size):
        """Host draw of one minibatch's chunks: (env [B], start [B]), start uniform in [0, length - chunk_size) of
        the env's retained transitions (ReplayBuffer.sample_chunk, irdqn.py:25: the newest transition is never a
        chunk's last), env uniform.  At n_envs = 1 this is the reference's one np.random.randint call.  Tests
        override it to inject recorded starts."""
        envs = np.zeros(batch_size, dtype=np.int64) if n_envs == 1 else np.random.randint(0, n_envs, batch_size)
        return envs, np.random.randint(0, length - chunk_size, batch_size)

    def _chunk_samples(self, E):
        """Device inputs of one update: samples [B][3] (env, last transition, L) plus done [B] of the last transition."""
        T, L, B = self.env.episode_length, self.history_len, self.minibatch_size
        length = min(self._added, self._cap)
        if length - L < 1:
            raise ValueError(f"replay holds {length} transitions per env; chunks of {L} need more "
                             f"(raise replay_start_size)")
        envs, starts = self._sample_chunks(E, length, B, L)
        last = (self._added - length) + np.asarray(starts, dtype=np.int64) + L - 1      # absolute transition index
        ntrans = self._ring_ep * T
        host = np.stack([np.asarray(envs, dtype=np.int64), last % ntrans, np.full(B, L), last % T == T - 1], 1)
        d = torch.from_numpy(host.astype(np.int32)).to(self.device)                    # one upload
        return d[:, :3].contiguous(), d[:, 3].to(torch.uint8)

    # --------------------------------------------------------------- update
    def _update(self, E):
        from d2dhip import rdqn
        T, L = self.env.episode_length, self.history_len
        samples, done = self._chunk_samples(E)
        e_idx, last = samples[:, 0].long(), samples[:, 1].long()
        _, qmax_t, _ = rdqn.q_values(self.target_network.data(), self._ring, samples, ring_episode=T, row_shift=1,
                                     want_q=False, want_action=False)
        action = self._act_ring[last, e_idx]                                             # [B][N]
        reward = self._rew_ring[last, e_idx].float().unsqueeze(1).expand(-1, self.n_agents).contiguous()
        _, loss = rdqn.grads(self.network.data(), self._ring, samples, L, action, reward, done, qmax_t, self.gamma,
                             self.loss_name, ring_episode=T, grads=self._grad_buffers(self.network.params))
        self.optimizer.step()
        self.losses.append(loss)
        self.n_updates += 1
        return loss

    def _sync_target(self):
        self.target_network.copy_from(self.network)
        self.n_syncs += 1

    # -------------------------------------------------------------- rollout
    def _act_slot(self, b, ring, row, S, act_out, mode, eps_rows=None, carry=None):
        """One d2d_rdqn_q_ex launch: every agent's action in every env on the window of the last S rows ending at
        `row`; with `carry`, on the previous slot's hidden state where this window extends that slot's by one row."""
        from d2dhip import rdqn
        E = b.E
        key = (id(b), E)
        if getattr(self, "_slot_key", None) != key:
            self._slot_key = key
            self._slot_samples = torch.zeros((E, 3), dtype=torch.int32, device=self.device)
            self._slot_samples[:, 0] = torch.arange(E, dtype=torch.int32, device=self.device)
        self._slot_samples[:, 1] = row
        self._slot_samples[:, 2] = S
        # the Parameters themselves, not .data(): their _version counters are part of the carry's tag
        rdqn.q_values(self.network.params, ring, self._slot_samples, mode=mode, eps_rows=eps_rows,
                      rng_step=b.rng_step, seed=self._policy_seed(), env_base=b.desc.env_base,
                      rng_offset=b.rng_off.data_ptr(), want_q=False, want_qmax=False, out={"action": act_out},
                      carry=carry, row=row, window=S)
        return act_out

    def _train_wave(self, b, ep0):
        """Episodes ep0 .. ep0 + E - 1 side by side, one per env, into the ring; returns per-env (score, reward)."""
        env, E, T, L = self.env, b.E, self.env.episode_length, self.history_len
        plans = [episode_plan(ep0 + e, **self._plan_kw()) for e in range(E)]
        # epsilon per env: above 1 = not ready, always explore (irdqn.py:151)
        eps_first = torch.tensor([p["eps_first"] if p["ready"] else 2.0 for p in plans], dtype=torch.float32,
                                 device=self.device)
        eps_rest = torch.tensor([p["eps"] if p["ready"] else 2.0 for p in plans], dtype=torch.float32,
                                device=self.device)
        slot = (self._added // T) % self._ring_ep
        r0, m0 = slot * (T + 1), slot * T
        carry = self._carry(b, "train")
        with torch.no_grad():
            b.reset(want_obs=True, out_obs=self._ring[r0])
            if carry is not None:
                carry.reset()     # a new episode: slot 0 recomputes whatever was written to the parameters since
            for t in range(T):
                act = self._act_slot(b, self._ring, r0 + t, min(t + 1, L), self._act_ring[m0 + t], "eps",
                                     eps_first if t == 0 else eps_rest, carry=carry)
                b.step(act, want_obs=True, out_obs=self._ring[r0 + t + 1], out_reward=self._rew_ring[m0 + t])
            env.timestep = b.timestep
            recv, disc = b.received.sum(1).double(), b.discarded.sum(1).double()
            score = (1 - disc / recv).cpu().tolist()
            reward = (self._rew_ring[m0:m0 + T].sum(0) * self.n_agents).cpu().tolist()   # sum_t rewards.sum()
        self._added += T
        for a in self.agents:
            a.epsilon = plans[-1]["eps"]
        return score, reward

    def train(self, n_episodes, early_stopping=True):
        from d2dhip import _lib
        _lib.refuse_ablation("iRDQN.train()")
        b = self._bind_env()
        b.spec.arrival_kinds()
        E = b.E
        n_waves = max(1, math.ceil(n_episodes / E))
        self._alloc_ring(b, n_waves)
        train_scores, test_list, reward_list = [], [], []
        for w in range(n_waves):
            ep0 = w * E
            scores, rewards = self._train_wave(b, ep0)
            n_here = min(E, n_episodes - ep0)
            done_eps = 0
            for name, ep in wave_events(ep0, E, n_episodes, **self._plan_kw()):
                if name == "test":
                    ts, tr = self.test(TEST_EPISODES)
                    test_list.append(ts)
                    reward_list.append(tr)
                    done_eps = ep - ep0 + 1
                    print(f"Episode: {ep}, Running reward: {rewards[ep - ep0]}, Test score: {ts}, "
                          f"eps: {epsilon_at(ep, self.initial_exploration_rate, self.final_exploration_rate)}, "
                          f"{len(train_scores) + done_eps}")
                    if early_stopping & (ts == 1):
                        print(f"Early stopping at episode {ep}")
                        train_scores += scores[:done_eps]
                        return train_scores, test_list, reward_list
                elif name == "update":
                    self._update(E)
                else:
                    self._sync_target()
            train_scores += scores[:n_here]
        return train_scores, test_list, reward_list

    # ----------------------------------------------------------------- test
    def test(self, n_episodes, verbose=False):
        """Greedy evaluation (irdqn.py:305-353): returns (1 - sum discarded / sum received over the episodes, mean
        episode score), the score of an episode being sum_t mean_agents max(reward, 0)."""
        return self._test(n_episodes, verbose=verbose)

    def _test(self, n_episodes, teacher=None, verbose=False):
        """test() body; `teacher` (parity tests) replays recorded env draws (BatchedLearnerBase._teacher_tensors;
        reference episode e * waves + w runs in env e, wave w), the actions stay the network's."""
        b = self._bind_env()
        if teacher is None and b.E == 1 and n_episodes > 1:
            b = self._episode_batch(n_episodes)
        env, E, T, L = self.env, b.E, self.env.episode_length, self.history_len
        s = b.spec
        waves = max(1, math.ceil(n_episodes / E))
        tf = self._teacher_tensors(teacher, b, waves) if teacher is not None else None
        ring = self._obs_ring(b, T + 1)
        carry = self._carry(b, "test")
        acts = torch.zeros((waves * T, E, s.N), dtype=b.action_buffer().dtype, device=self.device)
        rew = torch.zeros((waves * T, E), dtype=torch.int32, device=self.device)
        recv = torch.zeros((waves, E), dtype=torch.float64, device=self.device)
        disc = torch.zeros_like(recv)
        with torch.no_grad():
            for w in range(waves):
                b.reset(want_obs=True, out_obs=ring[0],
                        replay_arrivals=None if tf is None else tf["reset_arrivals"][w])
                if carry is not None:
                    carry.reset()
                for t in range(T):
                    i = w * T + t
                    act = self._act_slot(b, ring, t, min(t + 1, L), acts[i], "greedy", carry=carry)
                    b.step(act, want_obs=True, out_obs=ring[t + 1], out_reward=rew[i],
                           replay=None if tf is None else tf["replay"][i])
                env.timestep = b.timestep
                recv[w].copy_(b.received.sum(1))
                disc[w].copy_(b.discarded.sum(1))
        self._sync_episode_rng(b)
        # episodes env-major (env 0's waves, then env 1's, ...), the first n_episodes of them
        em = lambda x: x.t().reshape(-1)[:n_episodes]  # noqa: E731
        score = em(rew.clamp(min=0).view(waves, T, E).sum(1).double())
        self._last_test_actions = acts if teacher is not None else None
        recv_n, disc_n = em(recv).sum().item(), em(disc).sum().item()
        if verbose:
            print(f"received {recv_n}, discarded {disc_n}, scores {score.cpu().tolist()}")
        return 1 - disc_n / recv_n, score.mean().item()
