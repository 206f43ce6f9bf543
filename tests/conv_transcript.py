"""TEST-ONLY recorder of what ``dmcf_amd/utils/convolutions.py`` asks of ``dmcf_amd.ops``: every call of the functions in
WRAPPED, with its arguments bound to parameter names, and after every ContinuousConv / PointSampling call what the layer left
on itself.  A transcript is plain JSON; tests/test_conv_transcript_cpu.py and tests/test_gpu_conv_transcript.py hold the host
code to the transcripts recorded before its call preparation was folded.  The golden files (tests/golden/conv_transcript_*.json)
keep one line per record -- what it is and a hash of all of it (``digest``): the full transcripts of all cases are some
hundreds of KB; a comparison that fails prints the record found in full.

Encoding: a float as ``float.hex``; a tensor as the NAME of the layer input or weight it is (identity, not equality), any other
tensor as dtype, shape and the CRC-32 of its bytes; containers element-wise; any other object as its type name."""
import hashlib
import inspect
import json
import os
import zlib

import numpy as np
import torch

from dmcf_amd import ops
from dmcf_amd.utils import convolutions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WRAPPED = ("fixed_radius_search", "radius_search", "cconv_forward", "cconv_scatter_forward", "scatter_plan", "lattice_conv")
WEIGHTS = ("kernel", "bias", "dense")


class Recorder:
    """``Recorder(monkeypatch)`` wraps the ops functions and the two layers' ``forward``; ``.records`` is the transcript.
    Install it AFTER a backend such as tests/shims.py: it wraps whatever ``ops`` holds at that moment."""

    def __init__(self, monkeypatch, no_crc=()):
        self.records = []
        self.no_crc = no_crc  # arguments whose tensors are written without their CRC: bytes that no run fixes
        self.names = [{}]  # id(tensor) -> name, one frame per layer call in flight
        for name in WRAPPED:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name), inspect.signature(getattr(ops, name))))
        # (apply takes *args: its names are those of forward, without the context)
        params = list(inspect.signature(ops.ScatterConvFunction.forward).parameters.values())[1:]
        monkeypatch.setattr(ops.ScatterConvFunction, "apply", staticmethod(self._wrap(
            "ScatterConvFunction.apply", ops.ScatterConvFunction.apply, inspect.Signature(params))))
        for cls in (convolutions.ContinuousConv, convolutions.PointSampling):
            monkeypatch.setattr(cls, "forward", self._wrap_layer(cls.forward, inspect.signature(cls.forward)))

    def encode(self, v, crc=True):
        if isinstance(v, torch.Tensor):
            name = self.names[-1].get(id(v))
            if name is not None:
                return name
            t = {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)}
            if crc:
                t["crc"] = zlib.crc32(v.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy().tobytes())
            return t
        if isinstance(v, (bool, int, str)) or v is None:
            return v
        if isinstance(v, (float, np.floating)):
            return float(v).hex()
        if isinstance(v, (list, tuple)):
            return [self.encode(x, crc) for x in v]
        if isinstance(v, dict):
            return {str(k): self.encode(x, crc) for k, x in v.items()}
        return {"type": type(v).__name__}

    def _wrap(self, name, real, signature):
        def wrapped(*args, **kwargs):
            bound = signature.bind(*args, **kwargs).arguments  # (what the caller passed: defaults left out stay out)
            self.records.append({"call": name, "args": {k: self.encode(v, k not in self.no_crc) for k, v in bound.items()}})
            return real(*args, **kwargs)
        return wrapped

    def _wrap_layer(self, real, signature):
        def forward(layer, *args, **kwargs):
            given = signature.bind(layer, *args, **kwargs).arguments
            pending = {"accumulate_into": getattr(layer, "accumulate_into", None), "extra_bias": getattr(layer, "extra_bias", None)}
            frame = {id(v): k for k, v in list(given.items()) + list(pending.items()) if isinstance(v, torch.Tensor)}
            self.names.append(frame)
            rec = {"layer": layer.layer_name or type(layer).__name__, "inputs": sorted(frame.values())}
            try:
                frame.update({id(getattr(layer, w)): w for w in WEIGHTS if isinstance(getattr(layer, w, None), torch.Tensor)})
                try:
                    result = real(layer, *args, **kwargs)
                finally:  # (weights built by this very call)
                    frame.update({id(getattr(layer, w)): w for w in WEIGHTS if isinstance(getattr(layer, w, None), torch.Tensor)})
                rec["result"] = self.encode(result)
                rec["after"] = self.bookkeeping(layer, result)
            except Exception as e:
                rec["raised"] = {"type": type(e).__name__, "message": str(e)}
                raise
            finally:
                self.records.append(rec)
                self.names.pop()
            return result
        return forward

    @staticmethod
    def bookkeeping(layer, result):
        """What a call leaves on the layer ("absent": the class has no such attribute)."""
        d = {}
        nns = getattr(layer, "nns", "absent")
        d["nns"] = nns if nns is None or nns == "absent" else [type(nns).__name__, int(nns.neighbors_row_splits.shape[0]) - 1]
        d["_n_out_last"] = getattr(layer, "_n_out_last", "absent")
        d["_pairs_last"] = type(getattr(layer, "_pairs_last", None)).__name__
        cv = getattr(layer, "_conv_values", "absent")
        d["_conv_values"] = {k: v is None for k, v in cv.items()} if isinstance(cv, dict) else cv
        co = getattr(layer, "_conv_output", "absent")
        d["_conv_output"] = co if co is None or isinstance(co, str) else ("result" if co is result else "other")
        d["_direct_kernel"] = getattr(layer, "_direct_kernel", "absent")
        for k in ("accumulate_into", "extra_bias"):
            d[k + "_is_none"] = getattr(layer, k, None) is None
        return d


def digest(records):
    """The transcript as the golden files hold it, one short line per record: the function or layer, the first 12 hex digits of
    the SHA-1 of the record's canonical JSON, and for a refusal the exception in full."""
    lines = []
    for r in records:
        sha = hashlib.sha1(json.dumps(r, sort_keys=True, separators=(",", ":")).encode()).hexdigest()[:12]
        raised = r.get("raised") or r.get("case_raised")
        lines.append(f"{r.get('call') or r.get('layer') or ('step' if 'step' in r else 'case')} {sha}"
                     + (f" {raised['type']}: {raised['message']}" if raised else ""))
    return lines


def first_difference(golden, records):
    """Where the transcript departs from the golden digest (None: nowhere): the golden line, and the record found in full."""
    got = digest(records)
    for i, (a, b) in enumerate(zip(golden, got)):
        if a != b:
            return f"record {i}: golden {a!r}, got {b!r}: {json.dumps(records[i], sort_keys=True)}"
    return None if len(golden) == len(got) else f"{len(golden)} records != {len(got)}"


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def dump(transcripts, path):
    """The digests, one case per line: a changed case is one changed line."""
    lines = [f"{json.dumps(k)}: {json.dumps(digest(v))}" for k, v in transcripts.items()]
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")
