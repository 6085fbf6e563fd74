"""The disentangle regularisation's rows of the stream-order table (tests/stream_order.py), added from here as tests/png_stream_cases.py
adds the PNG decoder's.

tests/stream_order.py keeps one ``Case`` per operator and its census (tests/test_stream_order_host.py) wants a case for every export that
takes a stream.  ``mm_disentangle_inputs`` and ``mm_disentangle_forward / _backward`` are such exports; their cases are appended to
``stream_order.CASES`` when this module is imported, which tests/test_disentangle_host.py and tests/test_gpu_disentangle.py do -- both are
collected before the stream-order files, so the census, the decoy check and the delayed-side-stream test of
tests/test_gpu_stream_order.py run them with the other operators' cases."""
import torch

import stream_order as SO

B, V, HT, WT = 2, 5, 4, 8
BASE = ("textures", "vertices", "azimuths", "elevations", "distances", "biases", "delta_vertices")
FLIP = ("textures", "vertices")
JITTER = ("azimuths", "elevations", "distances", "biases", "delta_vertices")


def inputs_inputs(seed):
    g = SO.gen_of(seed)
    return torch.rand((B, 4, 8, 12), generator=g), torch.randint(1, 6, (B, 4), generator=g, dtype=torch.int32)


def inputs_op(Xa, boxes):
    f, e = SO.mod("disentangle").disentangle_inputs(Xa, boxes, value=0.5)
    return [f, e]


def check_inputs(Xa, boxes):
    assert Xa.dtype == torch.float32 and Xa.dim() == 4 and boxes.dtype == torch.int32 and tuple(boxes.shape) == (Xa.shape[0], 4)


def terms_inputs(seed):
    g = SO.gen_of(seed)
    r = lambda *s: torch.rand(*s, generator=g)

    def one():
        return {"textures": r(B, 3, HT, WT), "vertices": r(B, V, 3) - 0.5, "azimuths": r(B) * 360 - 180, "elevations": r(B) * 30,
                "distances": r(B) * 5 + 2, "biases": r(B, 2) * 0.6 - 0.3, "delta_vertices": (r(B, V, 3) - 0.5) * 0.2}
    Ae, Af, Aj = one(), one(), one()
    return Ae, {k: Af[k] for k in FLIP}, {k: Aj[k] for k in JITTER}


def terms_op(Ae, Af, Aj):
    Ae, Af, Aj = SO.leaves(Ae, BASE), SO.leaves(Af, FLIP), SO.leaves(Aj, JITTER)
    loss = SO.renderer(SO.S_RENDER).recon_disentangle(Ae, Af, Aj, 0.7, 0.3, azim=2.0)
    loss.backward()
    return [loss] + SO.grads(Ae, BASE) + SO.grads(Af, FLIP) + SO.grads(Aj, JITTER)


def check_terms(Ae, Af, Aj):
    assert tuple(Ae["textures"].shape) == (B, 3, HT, WT) == tuple(Af["textures"].shape) and tuple(Ae["vertices"].shape) == (B, V, 3)
    assert sorted(Af) == sorted(FLIP) and sorted(Aj) == sorted(JITTER)


CASES = [SO.case("disentangle_inputs (per-sample boxes)", inputs_inputs, inputs_op, ("mm_disentangle_inputs",), check=check_inputs),
         SO.case("recon_disentangle", terms_inputs, terms_op, ("mm_disentangle_forward", "mm_disentangle_backward"), check=check_terms)]
for c in CASES:
    if c.name not in SO.BY_NAME:
        SO.CASES.append(c)
        SO.BY_NAME[c.name] = c
