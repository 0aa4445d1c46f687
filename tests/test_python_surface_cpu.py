"""The Python surface of the fused calls without a GPU: what ShardedSbrOS forwards to its SbrOSVec - signature and arguments - and
what SbrEnv2Vec refuses, in which words.  No handle is created: a ShardedSbrOS is built with object.__new__ around a recorder,
and the refusals are called unbound."""
import inspect

import pytest

pytest.importorskip("torch")

FORWARDED = ("rollout", "rollout_actions", "lookahead", "lookahead_end", "lookahead_sampled", "lookahead_sampled_end", "branch_best",
             "mppi_update", "rollout_policy", "collect_policy", "lookahead_policy")

# one call per forwarded name: positional and keyword arguments mixed, at least one of them not the default
CALLS = {
    "rollout": ((5, 3), dict(return_actions=True)),
    "rollout_actions": (("tape",), dict(hold=2, return_rewards=True)),
    "lookahead": (("tape", 7), dict(return_best=True)),
    "lookahead_end": (("tape",), dict(n_steps=7, hold=3, return_rewards=True)),
    "lookahead_sampled": (("nominal", 16, "sampler"), dict(hold=2, return_actions=True)),
    "lookahead_sampled_end": (("nominal", 16, "sampler", 9), dict(return_best=True)),
    "branch_best": ((), dict(values="values")),
    "mppi_update": (("nominal", "returns", "sampler", 0.5), dict(shift=1, out="out")),
    "rollout_policy": (("policy", 12, 4), dict(noise_std=(0.25, 2.0), noise_seed=7, return_rewards=True)),
    "collect_policy": (("policy", 12), dict(hold=4, obs="obs", noise_seed=3)),
    "lookahead_policy": (("policy", 8, 12, 4, "obs"), dict(keep_mean=True, return_end=True)),
}

REFUSALS = {
    "rollout": "the fused random-policy rollout belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch",
    "lookahead": "the read-only lookahead belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch",
    "lookahead_sampled": "the sampled lookahead belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch",
    "lookahead_end": "the read-only lookahead belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch",
    "lookahead_sampled_end": "the sampled lookahead belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch",
    "lookahead_policy": "the closed-loop lookahead belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch",
    "collect_policy": "the fused policy collector belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch",
    "branch_best": "the winner of a lookahead's branches belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch",
    "mppi_update": "the MPPI tape update belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch",
}


@pytest.mark.parametrize("name", FORWARDED)
def test_a_shard_has_the_signature_it_forwards_to(name):
    from gym_sbr2_amd import SbrOSVec, ShardedSbrOS
    assert inspect.signature(getattr(ShardedSbrOS, name)) == inspect.signature(getattr(SbrOSVec, name))
    assert getattr(ShardedSbrOS, name) is not getattr(SbrOSVec, name)
    assert "rank's" in getattr(ShardedSbrOS, name).__doc__


class _Recorder:
    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        return lambda *args, **kwargs: self.seen.append((name, args, kwargs)) or ("result of", name)


@pytest.mark.parametrize("name", FORWARDED)
def test_a_shard_passes_its_arguments_through(name):
    from gym_sbr2_amd import SbrOSVec, ShardedSbrOS
    assert sorted(CALLS) == sorted(FORWARDED)
    sh = object.__new__(ShardedSbrOS)
    sh.env = _Recorder()
    args, kwargs = CALLS[name]
    assert getattr(sh, name)(*args, **kwargs) == ("result of", name)
    (seen_name, seen_args, seen_kwargs), = sh.env.seen
    assert seen_name == name
    sig = inspect.signature(getattr(SbrOSVec, name))
    want = sig.bind(None, *args, **kwargs)
    got = sig.bind(None, *seen_args, **seen_kwargs)
    assert got.arguments == want.arguments
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert not defaults or any(want.arguments[k] != d for k, d in defaults.items() if k in want.arguments), name   # the case itself


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_sbr_v2_refuses_in_these_words_before_it_looks_at_an_argument(name):
    from gym_sbr2_amd import SbrEnv2Vec
    with pytest.raises(NotImplementedError) as e:
        getattr(SbrEnv2Vec, name)(None)
    assert str(e.value) == REFUSALS[name]


def test_sbr_v2_refuses_these_nine_and_no_others():
    from gym_sbr2_amd import SbrEnv2Vec, SbrOSVec
    assert SbrEnv2Vec.rollout_actions is SbrOSVec.rollout_actions and SbrEnv2Vec.rollout_policy is SbrOSVec.rollout_policy
    own = {k for k, v in vars(SbrEnv2Vec).items() if callable(v) and not k.startswith("_")}
    assert own == set(REFUSALS) | {"reset", "step"}
