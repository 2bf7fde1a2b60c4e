"""Golden fixture for the HMM_DNN_ALI recipe (ml-vae_amd/models/HMM_DNN_ALI).

TEST INFRASTRUCTURE ONLY.  Runs only where a checkout of the reference is available; no test needs
it.  The reference recipe imports SpeechBrain's HMMAligner, VanillaNN and ctc_loss, which are not
vendored, so it cannot be run and there are no numeric fixtures from it: the float64 oracle
tests/hmm_np.py (checked against brute-force path enumeration and torch's CPU ctc_loss) takes
their place.  Only data is written: ``hmm_dnn_ali_yaml_keys.json``, the key names of the
reference's model.yaml (top level, ``modules:``, ``recoverables:``).

    python tests/golden/make_golden_hmm_dnn_ali.py <reference>/src
"""
import json
import os
import re
import sys

OUT_DIR = os.path.dirname(os.path.abspath(__file__))


def yaml_keys(ref_yaml):
    """Key names of the reference's model.yaml: top level, ``modules:`` and ``recoverables:``."""
    text = open(ref_yaml).read()
    top = re.findall(r"^([A-Za-z_][A-Za-z0-9_]*):", text, flags=re.M)

    def block(name, indent):
        body = re.search(rf"^{indent}{name}:\n((?:{indent}    \S.*\n?)+)", text, flags=re.M).group(1)
        return re.findall(r"^\s+([A-Za-z_][A-Za-z0-9_]*):", body, flags=re.M)

    return {"top_level": top, "modules": block("modules", ""), "recoverables": block("recoverables", "    ")}


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    keys = yaml_keys(os.path.join(sys.argv[1], "models", "HMM_DNN_ALI", "model.yaml"))
    path = os.path.join(OUT_DIR, "hmm_dnn_ali_yaml_keys.json")
    with open(path, "w") as f:
        json.dump(keys, f, indent=1)
    print("wrote", path, keys)
