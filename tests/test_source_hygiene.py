"""Housekeeping: the product kernels carry no measurement-only code paths (the ablation / timestamp variants of
k_sorted_pass behind profiles/r2_pass_ablation.txt lived beside the sources as a patch until round 4; the kernel they
patched has changed since -- its pixel loop runs on moments now -- and the patch went with it: the profile is the record)."""
import glob
import os

from conftest import PKG_DIR


def test_product_sources_have_no_ablation_hooks():
    for f in glob.glob(os.path.join(PKG_DIR, "csrc", "*")) + glob.glob(os.path.join(PKG_DIR, "host", "*")):
        text = open(f, errors="replace").read()
        assert "NLE_ABL_" not in text and "NLE_STAMP" not in text, f


# Environment switches whose variants were taken out (nothing but the switch reached them): no source may read them again
REMOVED_SWITCHES = ("NLE_HIST_UNTILED", "NLE_PROJECT_HIST", "NLE_EAGER_V", "NLE_APPLY_WITH_V", "NLE_HOST_ORTHO",
                    "NLE_PROJECT_CHUNKED", "NLE_NO_SORTED_EXPAND",
                    # the solver layer's tuning and measurement switches
                    "NLE_DEVICE_TRIDIAG", "NLE_WA_SERIAL", "NLE_NO_DEFLATE", "NLE_HOST_THREADS", "NLE_EIG_TQL",
                    "NLE_EIG_NO_BLOCK", "NLE_EIG_NO_INVIT", "NLE_EIG_THREADS", "NLE_PIN_THREADS", "NLE_EIG_TRACE",
                    "NLE_SYTRD_CW", "NLE_SYTRD_PROBE")


def test_product_sources_read_no_removed_switches():
    for f in glob.glob(os.path.join(PKG_DIR, "csrc", "*")) + glob.glob(os.path.join(PKG_DIR, "host", "*")):
        text = open(f, errors="replace").read()
        for name in REMOVED_SWITCHES:
            assert name not in text, (f, name)
