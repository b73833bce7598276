"""One table over all model classes of the HIP backend, through the public API only: create_model -> optimize -> metrics_fn -> save -> a fresh
create_model + load -> metrics again.  What each class computes is checked in its own module (test_gpu_backend.py, test_gpu_bound_variants.py,
test_gpu_multi_output.py, test_gpu_gpr.py, test_gpu_itergp.py); here every class goes through the same steps and the per-class scaffolding
(objective, predictor, optimiser loop, metrics, save / load) has to hold together for each of them.

The code under test is host code: N = 160 > M = 16 with several row blocks is all the library needs."""
import pytest

pytestmark = pytest.mark.gpu

N, N_TEST, D, M, STEPS = 160, 40, 3, 16, 3
RMSE_LPD = ["train/rmse", "train/nlpd", "test/rmse", "test/nlpd"]
CG = ["cg/steps", "cg/error"]
# class name -> (target columns, metric keys in the order they are reported, whether the class ever solves)
CASES = {
    "cglb": (1, CG + ["loss"] + RMSE_LPD, True),
    "cglbn2m": (1, CG + ["loss"] + RMSE_LPD, True),
    "cglbnm2": (1, CG + ["loss"] + RMSE_LPD, True),
    "sgpr": (1, ["elbo", "loss"] + RMSE_LPD, False),
    "sgprn2m": (1, ["elbo", "loss"] + RMSE_LPD, False),
    "gpr": (1, ["lml", "loss"] + RMSE_LPD, False),
    "itergp": (1, ["lml", "loss"] + CG + RMSE_LPD, True),
    "cglb-2-columns": (2, CG + ["loss"] + RMSE_LPD, True),
}


def _config(name):
    from cglb_amd.backend import config
    kernel = config.Matern32Config()
    name = name.split("-")[0]
    if name == "gpr":
        return config.GPRConfig(kernel), "scipy"
    if name == "itergp":
        return config.IterGPRConfig(kernel, num_probes=3, prec_size=M), "adam_0.1"
    return config.SGPR_CONFIGS[name](kernel=kernel, inducing_variable=config.InducingVariableConfig(M)), "scipy"


def _forget_what_save_does_not_keep(model, cfg):
    """`save` writes the parameters; the warm start of the solves and the state of the probe generator stay behind.  Brought to the state
    a freshly built model has: v = 0, and for itergp the generator re-seeded (fresh probes at every evaluation, not `deterministic_probes`)."""
    if hasattr(model, "v_vec"):
        model.v_vec.detach().zero_()
    if hasattr(model, "generator"):
        model.generator.manual_seed(cfg.seed)


def run_case(name, logdir, watch=None):
    """The steps of the table for one class.  `watch(model)` sees every model right after it is built."""
    from cglb_amd.backend import interface as backend
    from cglb_amd.backend.callbacks import Logger
    from cglb_amd.data import synthetic_problem
    backend.configure_backend(logdir=str(logdir))
    backend.set_default_float("fp64")
    backend.set_default_jitter(1e-6)
    columns = CASES[name][0]
    X, y, _Z = synthetic_problem(N + N_TEST, D, M, seed=5, P=columns)
    bundle = ((X[:N], y[:N]), (X[N:], y[N:]))
    cfg, optimizer = _config(name)
    model = backend.create_model(cfg, bundle[0])
    if watch is not None:
        watch(model)
    metrics_fn = backend.metrics_fn(model, bundle)
    logger = Logger(str(logdir), metrics_fn, lambda: backend.model_parameters(model), 1, include_feval_log=True, verbose=False)
    results = backend.optimize(model, bundle, STEPS, logger, optimizer)
    out = dict(results=results, logs=logger.logs, last_bound=model.last_bound, cg_stats=getattr(model, "cg_stats", None))
    out["trained"] = metrics_fn()
    out["params"] = backend.model_parameters(model)
    backend.save(model, str(logdir))
    _forget_what_save_does_not_keep(model, cfg)
    out["saved"] = metrics_fn()
    fresh = backend.create_model(cfg, bundle[0])
    if watch is not None:
        watch(fresh)
    backend.load(fresh, str(logdir / "model.json"))
    out["loaded"] = backend.metrics_fn(fresh, bundle)()
    out["loaded_cg_stats"] = getattr(fresh, "cg_stats", None)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_every_model_class_trains_reports_saves_and_loads(name, tmp_path):
    _columns, keys, solves = CASES[name]
    out = run_case(name, tmp_path)
    for which in ("trained", "saved", "loaded"):
        print(name, which, {k: repr(v) for k, v in out[which].items()})
    # the metric keys, in order; the CG statistics of the cglb classes are reported once a solve has run: not by the freshly loaded model
    assert list(out["trained"]) == keys and list(out["saved"]) == keys
    cglb = name.startswith("cglb")
    assert list(out["loaded"]) == [k for k in keys if not (cglb and k in CG)]
    # STEPS accepted steps, the metrics logged at each; the last evaluation of the run is the one behind the last logged loss
    assert len(out["logs"]["loss"]) == STEPS
    assert out["last_bound"] == -out["logs"]["loss"][-1]
    assert (out["cg_stats"] is not None) == solves
    assert (out["loaded_cg_stats"] is not None) == (name == "itergp")   # its metrics solve; those of the cglb classes reuse v as it is
    # the loaded model reproduces the saved one's metrics to the last bit (itergp: both from a generator re-seeded with the config's seed)
    for key, value in out["loaded"].items():
        assert value == out["saved"][key], (key, value, out["saved"][key])
