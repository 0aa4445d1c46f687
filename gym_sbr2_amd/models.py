"""Plant MODELS for the per-cycle lookahead under uncertain kinetics (SbrEnv2Vec.set_models, cycle_lookahead_models): a list of
configs that differ from a base config in the model fields only.  Host side, plain numpy; every check is libsbr_amd.so's own
(sbr_check_model), so what this module accepts is what sbr_set_models accepts."""
import ctypes as C

import numpy as np

from . import _capi

# the fourteen ASM1 rate constants of sbr_config, in the order of the struct: what perturbed() draws by default
MODEL_KINETICS = ("muH", "Ks", "Koh", "Kno", "bH", "eta_g", "eta_h", "kh", "Kx", "muA", "Knh", "bA", "Koa", "ka")
# every field in which a model may differ from the handle's config (include/sbr_amd.h): the yields and fractions, the rate
# constants, the oxygen saturation
MODEL_FIELDS = ("Ya", "Yh", "fp", "ixb", "ixp") + MODEL_KINETICS + ("So_sat",)


def copy_config(cfg):
    out = _capi.SbrConfig()
    C.memmove(C.byref(out), C.byref(cfg), C.sizeof(_capi.SbrConfig))
    return out


def set_table(env, models):
    """What set_models() of either vec env does: `models` (a PlantModels, a sequence of configs checked against env.cfg, or
    None / empty to drop the table) becomes the table of env's handle (sbr_set_models)."""
    import torch
    if models is not None and not isinstance(models, PlantModels):
        models = PlantModels(models, base=env.cfg) if len(models) else None
    n = 0 if models is None else len(models)
    with torch.cuda.device(env.device):
        _capi.check(env.lib.sbr_set_models(env._h, n, models.c_array() if n else None), env._h)


def table_size(env):
    """What num_models of either vec env reports (sbr_num_models)."""
    return int(env.lib.sbr_num_models(env._h))


class PlantModels:
    """An ensemble of plant models: `configs` is a sequence of _capi.SbrConfig, each a valid config that differs from `base`
    (default: the first of them) in the MODEL_FIELDS only - sbr_check_model decides, and a config that fails raises ValueError with
    the library's text, its index in front.  The configs are copied.  len(), indexing and iteration give the copies;
    c_array() the array sbr_set_models takes.

        models = PlantModels.perturbed(env.cfg, 8, rel_std=0.15, seed=1)
        env.set_models(models); ret = env.cycle_lookahead_models(candidates)          # 8 futures, one per model
    """

    def __init__(self, configs, base=None):
        configs = [copy_config(c) for c in configs]
        if not configs:
            raise ValueError("PlantModels needs at least one config")
        self.base = copy_config(configs[0] if base is None else base)
        lib = _capi.load()
        for m, cfg in enumerate(configs):
            if lib.sbr_check_model(C.byref(self.base), C.byref(cfg)) != 0:
                raise ValueError("model %d: %s" % (m, (lib.sbr_last_error(None) or b"?").decode()))
        self.configs = configs

    def __len__(self):
        return len(self.configs)

    def __getitem__(self, m):
        return self.configs[m]

    def __iter__(self):
        return iter(self.configs)

    def c_array(self):
        """(SbrConfig * len(self)) holding the models in order: the `models` argument of sbr_set_models."""
        arr = (_capi.SbrConfig * len(self.configs))()
        for m, cfg in enumerate(self.configs):
            C.memmove(C.byref(arr, m * C.sizeof(_capi.SbrConfig)), C.byref(cfg), C.sizeof(_capi.SbrConfig))
        return arr

    @classmethod
    def perturbed(cls, cfg, n, rel_std=0.1, seed=0, fields=MODEL_KINETICS, clip=2.0, keep_nominal=True):
        """`n` models around `cfg`: with keep_nominal model 0 is cfg itself; every other model multiplies each field of `fields`
        by exp(rel_std * z), the factor clipped to [1/clip, clip] - log-normal, so a rate constant stays positive and halving is as
        likely as doubling.  z comes from numpy.random.RandomState(seed).standard_normal((len(fields), n drawn models)): in field
        order, then model order, so a longer ensemble under the same seed does NOT extend a shorter one.  The default fields are
        the fourteen rate constants (MODEL_KINETICS); the yields and fractions (Ya, Yh, fp, ixb, ixp) and So_sat are perturbed
        only if named, and only MODEL_FIELDS may be named.
        VALIDITY DOMAIN.  cfg.scheme = 1 plans its Butcher-5 steps from the oxygen mode and ASSUMES every other mode (uptake of Ss,
        Snh, Sno; hydrolysis) has |lambda| * t_delta below about 2.5; with the reference's constants they stay below 1.0, and a
        plant with muH, muA, kh up to 4 x faster already misses the parity gate on some states (include/sbr_amd.h, sbr_config.scheme).
        Kinetics several times faster than the reference's are outside what either scheme was validated on: keep rel_std and
        clip moderate (the default clip of 2 stays inside the probed range), or check such a model against a fine solution first
        (sbr_eval_substeps with many substeps)."""
        n, clip, fields = int(n), float(clip), tuple(fields)
        if n < 1:
            raise ValueError("n must be >= 1")
        if not clip >= 1.0:
            raise ValueError("clip must be >= 1")
        for f in fields:
            if f not in MODEL_FIELDS:
                raise ValueError("%r is not a model field (%s)" % (f, ", ".join(MODEL_FIELDS)))
        drawn = n - 1 if keep_nominal else n
        z = np.random.RandomState(int(seed)).standard_normal((len(fields), drawn))
        factor = np.clip(np.exp(float(rel_std) * z), 1.0 / clip, clip)
        configs = [copy_config(cfg)] if keep_nominal else []
        for m in range(drawn):
            c = copy_config(cfg)
            for k, f in enumerate(fields):
                setattr(c, f, float(getattr(cfg, f) * factor[k, m]))
            configs.append(c)
        return cls(configs, base=cfg)
