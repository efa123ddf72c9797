"""Boundary check of the registry binding: the plugin lands in GraphGym's own ``layer_dict`` when GraphGym is importable.

graphgym_amd.registry binds, at import, to ``graphgym.register.layer_dict`` — the object GeneralLayer resolves layer_type
keys from (graphgym/models/layer.py:24,238).  The test runs a fresh interpreter with a stand-in ``graphgym.register`` on
PYTHONPATH (a module-level ``layer_dict`` and a ``register_layer`` that refuses duplicates: the interface the binding
uses) and checks that the engine's keys land in that very dictionary.  The duplicate-key messages are pinned by what the
reference's register.py:6-10 raises, stored in tests/golden/reference_register.json (make_register_golden.py)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_register.json")

STAND_IN = r"""
layer_dict = {}


def register_layer(key, module):
    if key in layer_dict:
        raise KeyError(key)
    layer_dict[key] = module
"""

SCRIPT = r"""
import json, sys
import graphgym.register as ref                      # the stand-in GraphGym registry
import graphgym_amd.registry as ours
import graphgym_amd.graphgym_plugin as plugin
out = {}
out["have_graphgym"] = ours.HAVE_GRAPHGYM
out["same_dict_object"] = ours.layer_dict is ref.layer_dict
out["keys_in_reference_dict"] = sorted(k for k in plugin.ALL_KEYS if ref.layer_dict.get(k) is plugin.ALL_KEYS[k])
try:
    ref.register_layer("gcnidconv", object)          # GraphGym's own duplicate check now sees our entry
    out["dup"] = None
except KeyError:
    out["dup"] = True
msgs = {}
for key in sys.argv[1:]:
    try:
        ours.register(key, 1, {key: 0})
    except KeyError as e:
        msgs[key] = str(e)
try:
    ours.register_layer("gcnidconv", object)          # through the shared dictionary
except KeyError as e:
    out["ours_dup_msg"] = str(e)
out["ours_msgs"] = msgs
layer = ref.layer_dict["Tfg-idgcn"](8, 16, bias=True)
out["params"] = sorted(n for n, _ in layer.named_parameters())
print(json.dumps(out))
"""


def test_plugin_lands_in_the_reference_registry(tmp_path):
    with open(GOLDEN) as f:
        ref_msgs = json.load(f)["duplicate_key_error"]
    pkg = tmp_path / "graphgym"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "register.py").write_text(STAND_IN)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path), ROOT]))
    r = subprocess.run([sys.executable, "-c", SCRIPT] + sorted(ref_msgs), env=env, capture_output=True, text=True,
                       timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["have_graphgym"] and out["same_dict_object"]
    assert len(out["keys_in_reference_dict"]) == 18
    assert out["dup"] is True
    assert out["ours_msgs"] == ref_msgs                # identical KeyError text (register.py:8)
    assert out["ours_dup_msg"] == ref_msgs["gcnidconv"]
    assert out["params"] == ["model.bias", "model.kernel", "model.kernel_id"]
