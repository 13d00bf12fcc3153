"""The official MANO_RIGHT.pkl -> the plain-array .npz alignsdf_amd.mano.ManoModel.from_npz reads.

    python tools/mano_pkl_to_npz.py MANO_RIGHT.pkl mano_right.npz [--flat_hand_mean]

The pickle (python 2, so read with latin1) holds chumpy objects; chumpy is not needed: an Unpickler maps every chumpy class to a stub
that keeps the object's state, and the array is the state's `x`.  J_regressor is a scipy sparse matrix and goes through scipy.
hands_mean is taken from the file unless --flat_hand_mean (then zeros: the reference's ManoLayer(flat_hand_mean=True); its ManoBranch
uses False).  The MANO licence does not allow redistributing the model: the .npz is for local use.
"""
import argparse
import pickle
import sys

import numpy as np

RIGHT_TIPS = (745, 317, 444, 556, 673)


class _ChumpyStub:
    """Stands in for any chumpy class: keeps whatever state the pickle hands over."""

    def __init__(self, *args, **kwargs):
        pass

    def __setstate__(self, state):
        self.__dict__.update(state if isinstance(state, dict) else {"state": state})


class _Unpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module == "chumpy" or module.startswith("chumpy."):
            return _ChumpyStub
        return super().find_class(module, name)


def as_array(value):
    """A plain ndarray of a pickle entry: an ndarray, a chumpy stub (its `x`), or a scipy sparse matrix."""
    if isinstance(value, _ChumpyStub):
        if hasattr(value, "x"):
            return np.asarray(value.x)
        if hasattr(value, "a") and hasattr(value, "idxs"):          # chumpy's Select (shapedirs is one): a.ravel()[idxs], reshaped
            picked = as_array(value.a).ravel()[np.asarray(value.idxs)]
            shape = getattr(value, "preferred_shape", None)
            return picked.reshape(shape) if shape is not None else picked
        raise ValueError("a chumpy object that is neither an array nor a selection (keys: %s)" % sorted(value.__dict__))
    if hasattr(value, "toarray"):
        return np.asarray(value.toarray())
    return np.asarray(value)


def convert(pkl_path, flat_hand_mean=False):
    """{name: array} of the model: the keys of ManoModel.from_npz."""
    with open(pkl_path, "rb") as f:
        data = _Unpickler(f, encoding="latin1").load()
    comps = as_array(data["hands_components"]).astype(np.float32)
    out = {
        "v_template": as_array(data["v_template"]).astype(np.float32).reshape(-1, 3),
        "shapedirs": as_array(data["shapedirs"]).astype(np.float32),
        "posedirs": as_array(data["posedirs"]).astype(np.float32),
        "J_regressor": as_array(data["J_regressor"]).astype(np.float32),
        "weights": as_array(data["weights"]).astype(np.float32),
        "hands_mean": np.zeros(comps.shape[1], np.float32) if flat_hand_mean else as_array(data["hands_mean"]).astype(np.float32),
        "comps": comps,
        "tips": np.asarray(RIGHT_TIPS, np.int32),
        "faces": as_array(data["f"]).astype(np.int32).reshape(-1, 3),
    }
    V = out["v_template"].shape[0]
    want = {"shapedirs": (V, 3, 10), "posedirs": (V, 3, 135), "J_regressor": (16, V), "weights": (V, 16), "hands_mean": (45,), "comps": (45, 45)}
    for k, shape in want.items():
        if out[k].shape != shape:
            raise ValueError("%s has shape %s, expected %s" % (k, out[k].shape, shape))
    parents = np.asarray(as_array(data["kintree_table"])[0]).astype(np.int64).tolist()
    if parents[1:] != [0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]:
        raise ValueError("a joint tree other than MANO's: %s" % parents)
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("pkl")
    p.add_argument("npz")
    p.add_argument("--flat_hand_mean", action="store_true")
    a = p.parse_args(argv)
    arrays = convert(a.pkl, a.flat_hand_mean)
    np.savez(a.npz, **arrays)
    print("%s: %d vertices, %d faces, |hands_mean| %.3f" % (a.npz, arrays["v_template"].shape[0], arrays["faces"].shape[0],
                                                           float(np.linalg.norm(arrays["hands_mean"]))))


if __name__ == "__main__":
    sys.exit(main())
