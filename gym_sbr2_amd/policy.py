"""The caller's policy for the fused closed-loop rollout (sbr_rollout_policy): a small MLP from the 18 observation values to
the two set-points, packed into the parameter block include/sbr_amd.h describes.  Packing is plain numpy and needs no GPU; the
block goes to the device when a rollout first asks for it."""
import ctypes as C
import warnings

import numpy as np

from . import _capi

WIDTHS = (32, 64)                     # hidden widths the library is built for; a narrower net is zero-padded to the next one
ACTIVATIONS = {"tanh": 0, "relu": 1}
SQUASHES = {"none": 0, "tanh": 1}


def param_count(n_hidden, width):
    """Floats in one policy's parameter block (sbr_policy_param_count of the C ABI, recomputed here so that packing needs no
    library)."""
    if n_hidden == 0:
        return _capi.NOBS * 2 + 2
    return (_capi.NOBS * width + width) + (width * width + width if n_hidden == 2 else 0) + (width * 2 + 2)


def _layers_of(module_or_pairs, activation):
    """[(W [out, in], b [out])] float32 and the hidden activation, from (W, b) pairs or a torch.nn.Sequential."""
    if hasattr(module_or_pairs, "children") and callable(module_or_pairs.children):       # a torch module
        import torch
        pairs, acts = [], []
        for m in module_or_pairs.children():
            if isinstance(m, torch.nn.Linear):
                if m.bias is None:
                    raise ValueError("every Linear of a policy needs a bias")
                pairs.append((m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()))
            elif isinstance(m, torch.nn.Tanh):
                acts.append((len(pairs), "tanh"))
            elif isinstance(m, torch.nn.ReLU):
                acts.append((len(pairs), "relu"))
            else:
                raise ValueError("a policy is a Sequential of Linear, Tanh and ReLU modules, not %s" % type(m).__name__)
        hidden = [a for k, a in acts if k < len(pairs)]
        if len(hidden) != max(len(pairs) - 1, 0) or [k for k, _ in acts][:len(hidden)] != list(range(1, len(pairs))):
            raise ValueError("every hidden Linear must be followed by exactly one activation")
        # a module behind the last Linear would be the squash, which is an argument of its own (with its action range): a
        # Sequential that carries one is not the net this class packs
        if len(acts) != len(hidden):
            raise ValueError("no module may follow the last Linear: the squash is the `squash` argument (with low / high)")
        if len(set(hidden)) > 1:
            raise ValueError("the hidden layers must share one activation")
        if hidden:
            activation = hidden[0]
        return pairs, activation
    return [(np.asarray(w), np.asarray(b)) for w, b in module_or_pairs], activation


class MlpPolicy:
    """An MLP policy 18 -> ... -> 2 with at most two hidden layers of at most 64 units.

    layers: [(W, b), ...] in torch.nn.Linear's convention (W [out, in]), or a torch.nn.Sequential of Linear and Tanh / ReLU
    modules.  activation: "tanh" | "relu" for the hidden layers.  squash: "tanh" maps the two outputs y to
    low + (high - low) * (tanh(y) + 1) / 2, i.e. mean + half-range * tanh(y); "none" uses y as the set-points.
    The env clips to its own action box afterwards either way."""

    def __init__(self, layers, activation="tanh", squash="tanh", low=(0.0, 0.0), high=(8.0, 15.0)):
        pairs, activation = _layers_of(layers, activation)
        if activation not in ACTIVATIONS:
            raise ValueError("activation must be one of %s" % sorted(ACTIVATIONS))
        if squash not in SQUASHES:
            raise ValueError("squash must be one of %s" % sorted(SQUASHES))
        if not 1 <= len(pairs) <= 3:
            raise ValueError("a policy has 1 to 3 Linear layers (at most two hidden ones), got %d" % len(pairs))
        fan_in = _capi.NOBS
        for k, (w, b) in enumerate(pairs):
            out = 2 if k == len(pairs) - 1 else w.shape[0] if w.ndim == 2 else -1
            if w.ndim != 2 or b.ndim != 1 or w.shape != (out, fan_in) or b.shape != (out,):
                raise ValueError("layer %d: expected W [%s, %d] and b [%s], got %s and %s"
                                 % (k, out if out > 0 else "out", fan_in, out if out > 0 else "out", w.shape, b.shape))
            if k < len(pairs) - 1 and not 1 <= out <= WIDTHS[-1]:
                raise ValueError("layer %d: hidden width %d is outside 1..%d" % (k, out, WIDTHS[-1]))
            fan_in = out
        self.n_hidden = len(pairs) - 1
        widest = max([w.shape[0] for w, _ in pairs[:-1]], default=0)
        self.width = next(h for h in WIDTHS if h >= widest)                   # the smallest build that fits
        if self.width > WIDTHS[0]:
            # measured: the 64-wide build costs ~150 us per decision, more than a torch net around step()
            warnings.warn("hidden width %d runs the 64-wide build of sbr_rollout_policy, whose net costs several times the 32-wide "
                          "one's per decision (DESIGN.md section 3.3): use hold > 1, or a net of at most 32 units" % widest,
                          RuntimeWarning, stacklevel=2)
        self.activation, self.squash = activation, squash
        low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
        if low.shape != (2,) or high.shape != (2,):
            raise ValueError("low and high are pairs (DO set-point, NO3 set-point)")
        if squash == "tanh":
            self.act_scale, self.act_bias = ((high - low) / 2).astype(np.float32), ((high + low) / 2).astype(np.float32)
        else:
            self.act_scale, self.act_bias = np.ones(2, np.float32), np.zeros(2, np.float32)
        self.layers = [(np.asarray(w, dtype=np.float32), np.asarray(b, dtype=np.float32)) for w, b in pairs]
        self.n_policies, self.envs_per_policy = 1, 0
        self.block = self.pack(self.width)[None, :]                            # [n_policies, param_count] float32
        self.members = [self]                                                  # a population (stack) lists its policies here
        self._dev = {}

    def pack(self, width):
        """This policy's parameter block for hidden width `width` (zero-padded): per layer W [out][in] row-major, then b."""
        if self.n_policies != 1:
            raise ValueError("pack() is a single policy's; a population's blocks are in .block (widened() re-packs them all)")
        if self.n_hidden and width < max(w.shape[0] for w, _ in self.layers[:-1]):
            raise ValueError("width %d is narrower than the net" % width)
        parts, fan_in = [], _capi.NOBS
        for k, (w, b) in enumerate(self.layers):
            out = 2 if k == self.n_hidden else width
            wp, bp = np.zeros((out, fan_in), np.float32), np.zeros((out,), np.float32)
            wp[:w.shape[0], :w.shape[1]] = w
            bp[:b.shape[0]] = b
            parts += [wp.ravel(), bp]
            fan_in = out
        blk = np.concatenate(parts)
        assert blk.size == param_count(self.n_hidden, width)
        return blk

    def widened(self, width):
        """The same policy (or population) packed for a wider build (64): same actions, bit for bit - padding is neutral."""
        q = self.__class__.__new__(self.__class__)
        q.__dict__.update(self.__dict__)
        q.width = int(width)
        q.block = np.stack([m.pack(q.width) for m in self.members])
        q.members = [q] if self.n_policies == 1 else self.members
        q._dev = {}
        return q

    @classmethod
    def stack(cls, policies, envs_per_policy):
        """A population: the env with GLOBAL id g runs policies[g // envs_per_policy].  The members share the architecture
        (hidden layers, activation, squash, action range); envs_per_policy is a multiple of 256."""
        policies = list(policies)
        if not policies:
            raise ValueError("an empty population")
        if int(envs_per_policy) < 256 or int(envs_per_policy) % 256:
            raise ValueError("envs_per_policy must be a positive multiple of 256")
        p0 = policies[0]
        for p in policies[1:]:
            if (p.n_hidden, p.activation, p.squash) != (p0.n_hidden, p0.activation, p0.squash) or \
                    not (np.array_equal(p.act_scale, p0.act_scale) and np.array_equal(p.act_bias, p0.act_bias)):
                raise ValueError("the members of a population must share hidden layers, activation, squash and action range")
        pop = cls.__new__(cls)
        pop.__dict__.update(p0.__dict__)
        pop.width = max(p.width for p in policies)
        if any(p.n_policies != 1 for p in policies):
            raise ValueError("the members of a population are single policies")
        pop.layers = None                                       # the members keep theirs
        pop.members = policies
        pop.block = np.stack([p.pack(pop.width) for p in policies])
        pop.n_policies, pop.envs_per_policy = len(policies), int(envs_per_policy)
        pop._dev = {}
        return pop

    def mean_f64(self, obs, member=0):
        """The action means [n, 2] of observations [n, 18], evaluated in float64 from the PACKED block (the checker's form of
        what the kernel computes in float32)."""
        blk = self.block[member].astype(np.float64)
        h, fan_in, at = np.asarray(obs, dtype=np.float64), _capi.NOBS, 0
        for k in range(self.n_hidden + 1):
            out = 2 if k == self.n_hidden else self.width
            w = blk[at:at + out * fan_in].reshape(out, fan_in)
            b = blk[at + out * fan_in:at + out * fan_in + out]
            at += out * fan_in + out
            h = h @ w.T + b
            if k < self.n_hidden:
                h = np.tanh(h) if self.activation == "tanh" else np.maximum(h, 0.0)
            fan_in = out
        if self.squash == "tanh":
            h = np.tanh(h)
        return self.act_bias.astype(np.float64) + self.act_scale.astype(np.float64) * h

    def device_block(self, device):
        """The packed block(s) as one contiguous float32 device tensor (made once per device)."""
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(np.ascontiguousarray(self.block)).to(device)
        return self._dev[key]

    def c_struct(self, device, noise_std=None, noise_seed=0):
        """struct sbr_policy for a launch on `device`."""
        std = (0.0, 0.0) if noise_std is None else tuple(float(v) for v in np.broadcast_to(np.asarray(noise_std, dtype=np.float64), (2,)))
        s = _capi.SbrPolicy()
        s.params = self.device_block(device).data_ptr()
        s.n_hidden, s.width = self.n_hidden, self.width
        s.activation, s.squash = ACTIVATIONS[self.activation], SQUASHES[self.squash]
        s.n_policies, s.envs_per_policy = self.n_policies, self.envs_per_policy
        s.act_scale = (C.c_float * 2)(*self.act_scale.tolist())
        s.act_bias = (C.c_float * 2)(*self.act_bias.tolist())
        s.noise_std = (C.c_float * 2)(*std)
        s.noise_seed = int(noise_seed) & (2 ** 64 - 1)
        return s
