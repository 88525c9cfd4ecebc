"""Environment.reset_where(mask) on the generic path (any scenario, CPU): rows of a full reset.

The yardstick is ``reset()`` of a twin env at the same state and generator states
(tests/_reset_where.py): inside the mask every batched state tensor equals the twin's, outside it
its own previous row, bit for bit; every generator ends where ``reset()`` leaves it; the returned
observations are those of the merged world; a following step agrees on the masked rows.
"""
import pytest
import torch

from tests import _reset_where as R
from vectorizedmultiagentsimulator_amd import make_env
from vectorizedmultiagentsimulator_amd.simulator.core import Agent, World
from vectorizedmultiagentsimulator_amd.simulator.scenario import BaseScenario

B = 5
SCENARIOS = ["balance", "transport", "discovery", "waterfall"]
CASES = [c[0] for c in R.mask_cases(B)]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_rows_of_a_full_reset_cpu(scenario, case):
    env, twin = R.twins(scenario, 2, B, "cpu")
    _, arg, mask = next(c for c in R.mask_cases(B) if c[0] == case)
    R.check_rows_of_full_reset(env, twin, arg, mask, "cpu")
    assert torch.equal(env.steps, torch.where(mask, 0.0, 3.0))
    R.check_next_step_agrees(env, twin, mask, "cpu")


@pytest.mark.parametrize("terminated_truncated", [False, True])
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_mask_none_resets_the_done_envs_cpu(scenario, terminated_truncated):
    """mask=None: the envs that are done -- here rows 1 and 3, truncated by a forced step count
    (plus whatever the scenario itself reports)."""
    env, twin = R.twins(scenario, 2, B, "cpu", max_steps=50, terminated_truncated=terminated_truncated)
    for e in (env, twin):
        e.steps[1] = 50
        e.steps[3] = 50
    d = twin.done()
    mask = (d[0] | d[1]) if terminated_truncated else d
    assert mask[1] and mask[3] and not mask.all()
    R.check_rows_of_full_reset(env, twin, None, mask, "cpu", return_dones=True, return_info=True)
    R.check_next_step_agrees(env, twin, mask, "cpu")


def test_index_tensor_and_bad_arguments_cpu():
    env, twin = R.twins("balance", 2, B, "cpu")
    mask = torch.tensor([False, True, False, False, True])
    R.check_rows_of_full_reset(env, twin, torch.tensor([4, 1, 4]), mask, "cpu")
    for bad in ([B], [-1], torch.tensor([0, B]), torch.zeros(B + 1, dtype=torch.bool), torch.zeros(B)):
        with pytest.raises(AssertionError):
            env.reset_where(bad)


def test_empty_mask_still_advances_the_generators_cpu():
    env, twin = R.twins("balance", 2, B, "cpu")
    g0 = R.get_rng("cpu")
    env.reset_where([])
    assert not R.same_rng(g0, R.get_rng("cpu"))


class _Toy(BaseScenario):
    """One agent; reset_world_at counts its calls in a Python int: state no row merge can split."""

    def make_world(self, batch_dim, device, **kwargs):
        world = World(batch_dim, device)
        world.add_agent(Agent(name="a"))
        self.resets = 0
        return world

    def reset_world_at(self, env_index=None):
        self.resets += 1
        a = self.world.agents[0]
        n = self.world.batch_dim
        pos = torch.zeros(n, 2, device=self.world.device).uniform_(-1, 1)
        a.set_pos(pos if env_index is None else pos[env_index], batch_index=env_index)

    def observation(self, agent):
        return agent.state.pos

    def reward(self, agent):
        return agent.state.pos[:, 0]


class _ToyWhere(_Toy):
    def reset_world_where(self, mask):
        self.resets += 1
        self.where_calls = getattr(self, "where_calls", 0) + 1
        a = self.world.agents[0]
        pos = torch.zeros(self.world.batch_dim, 2, device=self.world.device).uniform_(-1, 1)
        m = mask.unsqueeze(1)
        a.set_pos(torch.where(m, pos, a.state.pos), batch_index=None)
        a.set_vel(torch.where(m, 0.0, a.state.vel), batch_index=None)


def test_python_side_state_is_refused_cpu():
    env = make_env(_Toy(), num_envs=B, device="cpu", seed=0)
    env.step(env.get_random_actions())
    with pytest.raises(RuntimeError, match=r"_Toy\.resets.*fully reset"):
        env.reset_where([1])
    assert torch.equal(env.steps, torch.zeros(B))  # the world is fully reset, as the message says


def test_a_scenario_reset_world_where_is_used_cpu():
    env = make_env(_ToyWhere(), num_envs=B, device="cpu", seed=0)
    env.step(env.get_random_actions())
    env.step(env.get_random_actions())
    before = env.world.agents[0].state.pos.clone()
    obs = env.reset_where([1, 2])
    assert env.scenario.where_calls == 1
    mask = torch.tensor([False, True, True, False, False])
    pos = env.world.agents[0].state.pos
    assert torch.equal(pos[~mask], before[~mask]) and not torch.equal(pos[mask], before[mask])
    assert torch.equal(env.steps, torch.where(mask, 0.0, 2.0))
    assert torch.equal(obs[0], pos)
