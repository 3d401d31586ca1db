"""Shared by the GPU parity tests: the switches that make one kernel variant of the priority-stack family serve a small
batch, and the controller built under them."""
import casclik_amd as cc

SWITCHES = ("CLIK_LANES", "CLIK_JIT_VALUES", "CLIK_MODE_PARALLEL", "CLIK_FORCE_DYNAMIC")
# the switches that make a kernel variant serve a SMALL batch of the config-3 family (tests/test_capi.py holds the
# whole table); "quadv" is the library's own choice for a single-mode skill with forward kinematics
ENV = {
    "team4": {"CLIK_JIT_VALUES": "0"},
    "team4v": {},
    "mp2": {"CLIK_LANES": "1", "CLIK_JIT_VALUES": "0"},
    "mp4": {},                  # (the library's choice for a skill with two sets outside the config-3 family)
    "lane": {"CLIK_LANES": "1", "CLIK_JIT_VALUES": "0", "CLIK_MODE_PARALLEL": "0"},
    "lanev": {},                # (the library's choice beyond the team kernel's 16384 instances: see PAD)
    "quadv": {},
    "dynamic": {"CLIK_FORCE_DYNAMIC": "1"},
    "built-in": {},             # (a skill outside every shape-specialised family: the dynamic kernel by the library's choice)
}
# "lanev" serves the family only with the numbers compiled in, which the controller asks for when the team kernel is the
# skill's first choice - no switch makes it serve 257 instances.  Its cases run the smallest batch the library gives
# it, 16384 instances of the same distribution in front of the case's own (so the case's rows are the last waves and the
# ragged tail), and compare those.
PAD = {"lanev": 16384}


def set_switches(monkeypatch, values):
    """exactly `values` of the kernel switches in the environment, the others unset"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in values.items():
        monkeypatch.setenv(name, value)


def controller(spec, opts, batch, variant, monkeypatch):
    """the controller of the skill with the switches of `variant`; asserts that this variant serves `batch` instances
    (in front of which the caller launches PAD[variant] more, where the variant needs them)"""
    set_switches(monkeypatch, ENV[variant])
    ctrl = cc.PseudoInverseController(skill_spec=spec, options=None if opts is None else dict(opts))
    ctrl.setup_problem_functions()
    served = ctrl.kernel_variant(batch + PAD.get(variant, 0))
    if variant in ("dynamic", "built-in"):
        assert ctrl.kernel_name == "dynamic" and served == "dynamic/dynamic", served
    else:
        assert ctrl.kernel_name != "dynamic" and served.endswith("/" + variant), served
    return ctrl
