"""Host side of population-based training (no GPU needed): the new ABI symbols and struct layouts, every refusal of
frirl_hip_perturb_spec_check by column, and the argument checks frirl_hip_select_plan_device, frirl_hip_perturb_rows and the
frirl_hip_batch_evolve* calls make before they look for a device."""
import ctypes as C
import os
import subprocess

import pytest

import frirl_amd

NEW = ("frirl_hip_select_plan_device", "frirl_hip_perturb_spec_check", "frirl_hip_perturb_column_name", "frirl_hip_perturb_rows",
       "frirl_hip_batch_evolve_step", "frirl_hip_batch_evolve", "frirl_hip_batch_evolve_best_score")
EINVAL = -2
FULL = dict(alpha=(0.5, 2.0, 0.05, 0.9), gamma=(0.9, 1.1, 0.5, 0.999), weight_significant=(0.25, 4.0, 0.0, 0.5), epsilon=(0.5, 1.5, 0.01, 0.6),
            horizon=(0.5, 2.0, 1, 40), skip_rules=0.5, target=0.3, expected=0.7)


@pytest.fixture(scope="module")
def lib():
    frirl_amd.build()
    return frirl_amd.lib()


def test_new_symbols_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in frirl_amd.SIGNATURES, n
    for fn in ("select_plan_device", "perturb_rows", "perturb_spec", "batch_evolve_step", "batch_evolve"):
        assert callable(getattr(frirl_amd, fn)), fn
    assert callable(frirl_amd.Problem.select_plan_device) and callable(frirl_amd.Problem.perturb_rows)
    assert (frirl_amd.PLAN_OK, frirl_amd.PLAN_NAN, frirl_amd.PLAN_TOO_FEW) == (0, 1, 2)
    assert [lib.frirl_hip_perturb_column_name(c) for c in range(8)] == [n.encode() for n in frirl_amd.PERTURB_COLUMNS]
    assert lib.frirl_hip_perturb_column_name(8) is None and lib.frirl_hip_perturb_column_name(-1) is None


def test_struct_sizes_and_offsets_match_the_header(lib, tmp_path):
    """16 / 200 / 32 bytes, the offsets pinned here and compiled from include/frirl_hip.h by the C compiler."""
    I, P, R = frirl_amd.SelectInfo, frirl_amd.PerturbSpec, frirl_amd.EvolveResult
    assert C.sizeof(I) == 16 and (I.N.offset, I.status.offset, I.best.offset, I.bad_agent.offset) == (0, 4, 8, 12)
    assert C.sizeof(P) == 200
    assert (P.columns.offset, P.reserved.offset, P.seed.offset, P.down.offset, P.up.offset, P.lo.offset, P.hi.offset, P.flip.offset) == (0, 4, 8, 16, 56, 96, 136, 176)
    assert C.sizeof(R) == 32
    assert (R.best.offset, R.parents.offset, R.replaced.offset, R.perturbed.offset, R.rules_copied.offset, R.generation.offset, R.plan_status.offset) == (0, 4, 8, 12, 16, 24, 28)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "frirl_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(frirl_hip_select_info), sizeof(frirl_hip_perturb_spec), sizeof(frirl_hip_evolve_result),\n'
                   '         offsetof(frirl_hip_select_info, bad_agent), offsetof(frirl_hip_perturb_spec, seed), offsetof(frirl_hip_perturb_spec, up),\n'
                   '         offsetof(frirl_hip_perturb_spec, hi), offsetof(frirl_hip_perturb_spec, flip), offsetof(frirl_hip_evolve_result, rules_copied),\n'
                   '         offsetof(frirl_hip_evolve_result, generation), offsetof(frirl_hip_evolve_result, plan_status), FRIRL_HIP_PERTURB_HORIZON, FRIRL_HIP_PERTURB_EXPECTED);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu99", "-I", os.path.join(frirl_amd.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [16, 200, 32, 12, 8, 56, 136, 176, 16, 24, 28, 4, 7]


def test_perturb_spec_builds_the_struct(lib):
    spec = frirl_amd.perturb_spec(seed=7, **FULL)
    assert spec.columns == 255 and spec.seed == 7 and spec.reserved == 0
    assert (spec.down[4], spec.up[4], spec.lo[4], spec.hi[4]) == (0.5, 2.0, 1.0, 40.0) and list(spec.flip) == [0.5, 0.3, 0.7]
    assert lib.frirl_hip_perturb_spec_check(C.byref(spec)) == 0
    assert frirl_amd.perturb_spec(epsilon=FULL["epsilon"]).columns == 1 << 3
    with pytest.raises(TypeError, match="qdiff_pos_boundary"):
        frirl_amd.perturb_spec(qdiff_pos_boundary=(0.5, 2.0, 0.0, 1.0))


def refused(lib, spec):
    assert lib.frirl_hip_perturb_spec_check(C.byref(spec)) == EINVAL
    return lib.frirl_hip_last_error().decode()


def test_every_refusal_of_the_spec_check_names_its_column(lib):
    nan, inf = float("nan"), float("inf")
    for name in frirl_amd.PERTURB_COLUMNS[:5]:
        dn, up, lo, hi = FULL[name]
        bad = [(1 / 32, up, lo, hi), (dn, 17.0, lo, hi), (nan, up, lo, hi), (dn, inf, lo, hi), (dn, up, hi, lo) if lo != hi else None, (dn, up, nan, hi),
               (dn, up, lo, inf), (dn, up, -inf, hi)]
        for v in filter(None, bad):
            msg = refused(lib, frirl_amd.perturb_spec(**{name: v}))
            assert msg.startswith(f"frirl_hip_perturb_spec_check: {name}: "), (name, v, msg)
        assert lib.frirl_hip_perturb_spec_check(C.byref(frirl_amd.perturb_spec(**{name: (1 / 16, 16.0, lo, lo)}))) == 0, name
    for name, v in (("epsilon", (0.5, 2.0, -0.1, 0.5)), ("epsilon", (0.5, 2.0, 0.0, 1.5)), ("weight_significant", (0.5, 2.0, -1e-9, 0.5)),
                    ("horizon", (0.5, 2.0, -1, 5)), ("horizon", (0.5, 2.0, 0, (1 << 30) + 1))):
        assert refused(lib, frirl_amd.perturb_spec(**{name: v})).startswith(f"frirl_hip_perturb_spec_check: {name}: "), (name, v)
    assert lib.frirl_hip_perturb_spec_check(C.byref(frirl_amd.perturb_spec(horizon=(0.5, 2.0, 0, 1 << 30), epsilon=(0.5, 2.0, 0.0, 1.0)))) == 0
    for name in frirl_amd.PERTURB_COLUMNS[5:]:
        for p in (-0.1, 1.1, nan):
            assert refused(lib, frirl_amd.perturb_spec(**{name: p})).startswith(f"frirl_hip_perturb_spec_check: {name}: "), (name, p)
    # what is not enabled is not looked at
    spec = frirl_amd.perturb_spec(alpha=FULL["alpha"])
    spec.down[1], spec.flip[2] = nan, 9.0
    assert lib.frirl_hip_perturb_spec_check(C.byref(spec)) == 0
    spec.reserved = 1
    assert "reserved" in refused(lib, spec)
    spec.reserved, spec.columns = 0, 256
    assert "columns" in refused(lib, spec)
    assert lib.frirl_hip_perturb_spec_check(None) == EINVAL and "NULL" in lib.frirl_hip_last_error().decode()


def test_plan_device_checks_its_arguments_before_the_device(lib):
    """FRIRL_HIP_EINVAL (-2) where a machine without a GPU would otherwise answer FRIRL_HIP_ENODEV (-1)."""
    buf = (C.c_double * 64)()
    p = C.addressof(buf)

    def call(scores=p, E=4, eligible=None, parents=1, replace=1, src=p, rank=p, info=p):
        assert lib.frirl_hip_select_plan_device(scores, E, eligible, parents, replace, src, rank, info, None) == EINVAL
        return lib.frirl_hip_last_error().decode()

    for kw, word in ((dict(scores=None), "NULL"), (dict(src=None), "NULL"), (dict(rank=None), "NULL"), (dict(info=None), "NULL"), (dict(E=0), "E=0"),
                     (dict(parents=0), "parents=0"), (dict(replace=-1), "replace=-1"), (dict(parents=2, replace=3), "parents=2 + replace=3")):
        msg = call(**kw)
        assert msg.startswith("frirl_hip_select_plan_device: ") and word in msg, (kw, msg)
    assert not any(buf), "a refused plan writes nothing"


def test_perturb_rows_checks_its_arguments_before_the_device(lib):
    buf = (C.c_int32 * 16)()
    p = C.addressof(buf)
    spec = frirl_amd.perturb_spec(alpha=FULL["alpha"])
    fn = lib.frirl_hip_perturb_rows
    assert fn(None, 0, 4, p, None, None, None, None, None, None) == EINVAL and "NULL" in lib.frirl_hip_last_error().decode()
    assert fn(C.byref(spec), 0, 4, None, None, None, None, None, None, None) == EINVAL and "NULL" in lib.frirl_hip_last_error().decode()
    assert fn(C.byref(spec), 0, 0, p, None, None, None, None, None, None) == EINVAL and "E=0" in lib.frirl_hip_last_error().decode()
    bad = frirl_amd.perturb_spec(alpha=(0.5, 32.0, 0.0, 1.0))
    assert fn(C.byref(bad), 0, 4, p, None, None, None, None, None, None) == EINVAL and "alpha" in lib.frirl_hip_last_error().decode()


def test_batch_evolve_calls_refuse_a_null_batch(lib):
    res = frirl_amd.EvolveResult()
    assert lib.frirl_hip_batch_evolve_step(None, 1, None, 1, 1, 0, None, C.byref(res)) == EINVAL
    assert lib.frirl_hip_last_error() == b"frirl_hip_batch_evolve_step: NULL batch"
    assert lib.frirl_hip_batch_evolve(None, 1, 1, 1, None, 1, 1, 0, None, None) == EINVAL
    assert lib.frirl_hip_last_error() == b"frirl_hip_batch_evolve: NULL batch"
    assert lib.frirl_hip_batch_evolve_best_score(None, None, None) == EINVAL


DEMO = os.path.join(frirl_amd.PKG_DIR, "lib", "frirl_demo")
SELECT = ["--env", "mountaincar", "--agents", "8", "--select-episodes", "4", "--select-parents", "2", "--select-replace", "3"]


@pytest.mark.parametrize("flags,word", [
    (["--select-perturb", "alpha:0.8:1.25:0.05:1.0"], "go with --select G"),
    (["--select-flip", "skip_rules:0.5"], "go with --select G"),
    (["--select-seed", "3"], "go with --select G"),
    (["--select", "2", "--select-perturb", "alpha:0.8:1.25:0.05"], "col:down:up:lo:hi"),
    (["--select", "2", "--select-perturb", "qdiff_pos_boundary:0.8:1.25:0.05:1.0"], "col:down:up:lo:hi"),
    (["--select", "2", "--select-perturb", "skip_rules:0.8:1.25:0.05:1.0"], "col:down:up:lo:hi"),
    (["--select", "2", "--select-flip", "alpha:0.5"], "col:p"),
    (["--select", "2", "--select-seed", "x"], "whole number"),
    (["--select", "2", "--select-perturb", "alpha:0.8:1.25:0.05:1.0"], "give --hparams FILE"),
    (["--select", "2", "--select-perturb", "epsilon:0.8:1.25:0.05:1.0"], "give --explore FILE"),
    (["--select", "2", "--select-flip", "target:0.5"], "neither --target nor --expected"),
    (["--select", "2", "--select-perturb", "alpha:0.8:32:0.05:1.0"], "alpha: up 32"),
])
def test_demo_refuses_perturbation_flags_it_cannot_honour(lib, flags, word, tmp_path):
    """Exit status 2 and the cause on stderr, before any device is touched."""
    r = subprocess.run([DEMO] + SELECT + flags, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr, (r.returncode, r.stderr[:400])
