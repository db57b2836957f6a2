"""Seeded sequences of calls of ONE stencil object, a plain model of which of them a launch-plan cache may serve, and a census of
the cache transitions a set of sequences reaches.  Test infrastructure; imports no product code and (at import) no torch.

A sequence works on small pools, so that objects, domains and scalars recur: per field ``SLOTS`` array objects, each with
``BUFFERS`` buffers of one shape it can point at (the last with a padded pitch), three domains, two origins per field, a palette of
scalars, seven streams (index 0: the default stream).  A step is the previous call with one thing changed, after an optional
mutation of an array; the step kinds are the names in ``KINDS``.

The model restates the contract, not the product's code: a plan may be reused only if stream (generic executor), domain, origins,
the identity, address, shape and strides of every array and the bits of every scalar in its parameter's dtype all match a live
entry.  What it does take from the product are the two capacities and their eviction order (8 plans, first in first out; scratch for
one domain per stream and at most 4 streams, oldest first), since a test cannot say what an eviction costs without them."""

from __future__ import annotations

import copy
import dataclasses
import random
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

SLOTS = 3  # array objects per field
BUFFERS = 3  # buffers per array object: 0 and 1 alike, 2 with a padded pitch
STREAMS = 7  # index 0: the default stream; six more, which is more than the scratch buffers kept
PLAN_CAPACITY = 8
SCRATCH_STREAMS = 4
FLOAT_PALETTE = [0.0, -0.0, 1.5, -2.0, 1, True, 0.1, np.float32(0.1), float("inf"), float("nan")]
#: ... for random programs, whose casts and comparisons are defined for finite values only
FINITE_PALETTE = [0.0, -0.0, 1.5, -2.0, 1, True, 0.1, np.float32(0.1)]
INT_PALETTE = [0, 1, True, -3]
PATHS = ["call", "call+info", "frozen", "frozen+info"]
#: the mutations and special calls of the issue, each a step kind with a name ...
MUTATIONS = ["refill", "replace", "repoint", "repitch", "alias", "refused", "churn", "overflow"]
#: ... and the plain changes between two calls
CHANGES = ["repeat", "recall", "scalar", "origin", "domain", "stream", "arrays", "path"]
KINDS = MUTATIONS + CHANGES
CAUSES = ["scalar bits", "address", "strides", "origin", "domain", "stream", "dead object", "capacity eviction", "scratch eviction"]


@dataclasses.dataclass(frozen=True)
class Spec:
    """What a sequence needs to know of the object under test."""

    name: str
    fields: Tuple[str, ...]
    domains: Tuple[Tuple[int, int, int], ...]
    float_params: Dict[str, str] = dataclasses.field(default_factory=dict)  # name -> dtype name
    int_params: Dict[str, str] = dataclasses.field(default_factory=dict)
    generic: bool = True  # generic executor: the stream and the scalars are part of a plan
    scratch: bool = False  # ... with temporaries in scratch memory
    alias: Optional[Tuple[str, str]] = None  # (written, read) that may be one array
    refusals: Tuple[Tuple[str, str], ...] = ()  # pairs of fields that must not be one array
    palette: Tuple[Any, ...] = tuple(FLOAT_PALETTE)
    own_scalars: Dict[str, Any] = dataclasses.field(default_factory=dict)  # the values a random program was made with
    keyed: Optional[Tuple[str, ...]] = None  # the fields a plan holds (default: all)

    @property
    def params(self):
        return {**self.float_params, **self.int_params}

    def causes(self) -> List[str]:
        """The causes of a miss this object can have."""
        out = ["address", "strides", "origin", "domain", "dead object", "capacity eviction"]
        if self.generic:
            out += ["stream"] + (["scalar bits"] if self.params else []) + (["scratch eviction"] if self.scratch else [])
        return out

    def kinds(self) -> List[str]:
        out = [k for k in KINDS if k != "scalar" or self.params]
        return [k for k in out if (k != "alias" or self.alias) and (k != "refused" or self.refusals)]


def scalar_bits(dtype: str, value) -> bytes:
    return np.dtype(dtype).type(value).tobytes()


@dataclasses.dataclass
class Step:
    kind: str
    path: str
    stream: int
    domain: Tuple[int, int, int]
    origin: Dict[str, int]  # field -> 0 | 1 (1: the origin with a lead)
    slots: Dict[str, int]  # field -> array object
    scalars: Dict[str, Any]
    mutation: Optional[Tuple[str, str, int, int]] = None  # (kind, field, slot, new buffer) before the call
    same_as: Optional[Tuple[str, str]] = None  # alias / refused: (field, the field whose array it is given)
    refused: bool = False
    # the model's verdict
    hit: bool = False
    cause: Optional[str] = None
    may_miss: bool = False


class Model:
    """The caches of one object, as the contract and the two capacities define them."""

    def __init__(self, spec: Spec):
        self.spec = spec
        self.uid = {(f, s): s for f in spec.fields for s in range(SLOTS)}  # identity of the object in a slot
        self.next_uid = SLOTS
        self.buffer = {(f, s): 0 for f in spec.fields for s in range(SLOTS)}
        self.generation = {(f, s): 0 for f in spec.fields for s in range(SLOTS)}  # buffers of a replaced object are new ones
        self.plans: Dict[Any, bool] = {}  # key -> one of its arrays was re-pointed or replaced since the entry was made
        self.scratch: List[Tuple[int, Tuple[int, int, int]]] = []  # (stream, domain), oldest first
        self.gone: Dict[Any, str] = {}  # key -> what evicted it

    # -- mutations
    def mutate(self, kind, field, slot, buffer):
        if kind == "replace":
            self.uid[field, slot] = self.next_uid
            self.next_uid += 1
            self.generation[field, slot] += 1
            self.buffer[field, slot] = 0
        elif kind in ("repoint", "repitch"):
            self.buffer[field, slot] = buffer
        if kind != "refill":
            for key in self.plans:
                if any(a[0] == field and a[1] == slot for a in key[3]):
                    self.plans[key] = True

    def key(self, step: Step):
        arrays = []
        for f in (self.spec.keyed or self.spec.fields):
            g = step.same_as[1] if step.same_as and step.same_as[0] == f else f
            s = step.slots[g]
            b = self.buffer[g, s]
            arrays.append((g, s, self.uid[g, s], (self.generation[g, s], b), "padded" if b == BUFFERS - 1 else "plain"))
        bits = tuple(scalar_bits(dt, step.scalars[p]) for p, dt in self.spec.params.items()) if self.spec.generic else ()
        return (step.stream if self.spec.generic else None, step.domain, tuple(step.origin[f] for f in (self.spec.keyed or self.spec.fields)),
                tuple(arrays), bits)

    def _cause(self, key) -> str:
        if key in self.gone:
            return self.gone[key]
        best = None
        for other in self.plans:
            diff = []
            if other[4] != key[4]:
                diff.append("scalar bits")
            for a, b in zip(other[3], key[3]):
                if a[:2] != b[:2] or a[2] != b[2]:
                    diff.append("dead object" if a[:2] == b[:2] else "arrays")
                elif a[3] != b[3]:
                    diff.append("strides" if a[4] != b[4] else "address")
            if other[2] != key[2]:
                diff.append("origin")
            if other[1] != key[1]:
                diff.append("domain")
            if other[0] != key[0]:
                diff.append("stream")
            if best is None or len(diff) < len(best):
                best = diff
        if not best:
            return "cold"
        order = CAUSES + ["arrays"]
        return min(best, key=order.index)

    def _drop_stream(self, stream, why):
        for key in [k for k in self.plans if k[0] == stream]:
            del self.plans[key]
            self.gone[key] = why
        self.scratch = [e for e in self.scratch if e[0] != stream]

    def call(self, step: Step) -> None:
        key = self.key(step)
        if key in self.plans:
            step.hit, step.cause, step.may_miss = True, None, self.plans[key]
            return
        step.hit, step.cause = False, self._cause(key)
        if self.spec.scratch and (step.stream, step.domain) not in self.scratch:  # (a refused call gets as far as this, too)
            self._drop_stream(step.stream, "scratch eviction")
            streams = list(dict.fromkeys(s for s, _ in self.scratch))
            for old in streams[:max(0, len(streams) - (SCRATCH_STREAMS - 1))]:
                self._drop_stream(old, "scratch eviction")
            self.scratch.append((step.stream, step.domain))
        if step.refused and self.spec.generic:
            return  # refused while the plan was prepared: nothing kept
        if len(self.plans) >= PLAN_CAPACITY:
            first = next(iter(self.plans))
            del self.plans[first]
            self.gone[first] = "capacity eviction"
        self.plans[key] = False
        self.gone.pop(key, None)


def make_sequence(spec: Spec, seed: int, length: int) -> List[Step]:
    """``length`` steps for ``spec``; the model's verdict is filled in."""
    r = random.Random(f"{spec.name}/{seed}")
    model = Model(spec)
    kinds = spec.kinds()

    def pick_scalars():
        out = {}
        for p in spec.float_params:
            out[p] = r.choice(list(spec.palette) + ([spec.own_scalars[p]] if p in spec.own_scalars else []))
        for p in spec.int_params:
            out[p] = r.choice(INT_PALETTE)
        return out

    prev = Step("arrays", "call", 0, spec.domains[0], {f: 0 for f in spec.fields}, {f: 0 for f in spec.fields}, pick_scalars())
    steps: List[Step] = []
    history: List[Step] = []  # ordinary calls, to come back to
    followed = set()  # the causes of a miss that the same call has followed at once
    pending: List[Tuple[str, Step]] = []  # steps that follow by plan: the return after a churn, the repeat after a miss
    # every kind in turn first, then at random: a short sequence reaches them all
    long = ("churn", "overflow")  # (five and ten steps each: once per sequence)
    special = [k for k in kinds if k in MUTATIONS and k not in long]
    agenda = [k for k in kinds if k not in long] + special + ["scalar", "zero"] * bool(spec.float_params) \
        + ["scalar"] * bool(spec.params)
    r.shuffle(agenda)
    agenda += [k for k in kinds if k in long]  # (taken from the end)
    kinds = [k for k in kinds if k not in long]
    while len(steps) < length:
        if pending:
            kind, base = pending.pop(0)
            base = base or prev
        else:
            kind, base = (agenda.pop() if agenda else r.choice(kinds)), prev
        step = dataclasses.replace(base, kind=kind, mutation=None, same_as=None, refused=False, origin=dict(base.origin),
                                   slots=dict(base.slots), scalars=dict(base.scalars))
        field = r.choice(spec.fields)
        if kind == "recall" and history:
            old = r.choice(history[-12:])
            step = dataclasses.replace(old, kind=kind, origin=dict(old.origin), slots=dict(old.slots), scalars=dict(old.scalars))
        elif kind in ("zero", "negative zero"):  # the pair a key of VALUES cannot tell apart
            p = next(iter(spec.float_params))
            step.scalars[p] = 0.0 if kind == "zero" else -0.0
            if kind == "zero":
                pending = [("negative zero", step), ("repeat", None)]
            step.kind = "scalar"
        elif kind == "scalar":
            p = r.choice(list(spec.params))
            old_bits = scalar_bits(spec.params[p], step.scalars[p])
            pool = list(spec.palette) if p in spec.float_params else INT_PALETTE
            # half of the time the neighbour in the palette (0.0 -> -0.0, 1 -> True, 0.1 -> float32(0.1)), else a value with
            # other bits, one the cache does not hold where there is one
            at = [n for n, v in enumerate(pool) if scalar_bits(spec.params[p], v) == old_bits]
            if at and r.random() < 0.5:
                step.scalars[p] = pool[(at[0] + 1) % len(pool)]
            else:
                others = [v for v in pool if scalar_bits(spec.params[p], v) != old_bits]
                r.shuffle(others)
                fresh = [v for v in others if model.key(dataclasses.replace(step, scalars={**step.scalars, p: v})) not in model.plans]
                step.scalars[p] = (fresh or others)[0]
        elif kind == "origin":
            step.origin[field] = 1 - step.origin[field]
        elif kind == "domain":
            step.domain = r.choice([d for d in spec.domains if d != step.domain])
        elif kind == "stream":
            step.stream = r.choice([s for s in range(STREAMS) if s != step.stream])
        elif kind == "arrays":
            step.slots[field] = r.choice([s for s in range(SLOTS) if s != step.slots[field]])
        elif kind == "path":
            pass  # the same call by another path, below
        elif kind in ("refill", "replace"):
            step.mutation = (kind, field, step.slots[field], 0)
        elif kind in ("repoint", "repitch"):
            plain = [f for f in spec.fields if model.buffer[f, step.slots[f]] != BUFFERS - 1]
            if kind == "repoint" and plain:
                field = r.choice(plain)
            now = model.buffer[field, step.slots[field]]
            if kind == "repoint" and now == BUFFERS - 1:
                step.kind = kind = "repitch"  # off the padded buffer: the strides change with the address
            new = (1 - now) if kind == "repoint" else (BUFFERS - 1 if now != BUFFERS - 1 else 0)
            step.mutation = (kind, field, step.slots[field], new)
        elif kind == "alias":
            step.same_as = spec.alias
            step.origin[spec.alias[0]] = step.origin[spec.alias[1]]  # the same elements, not a shifted view
        elif kind == "refused":
            step.same_as, step.refused, step.path = r.choice(spec.refusals), True, "frozen"
        elif kind == "churn":  # SCRATCH_STREAMS other streams, then this one again
            home = dataclasses.replace(step)
            for _ in range(20):  # an order of visits after which the scratch of this stream is gone, where there is one
                others = r.sample([s for s in range(STREAMS) if s != step.stream], SCRATCH_STREAMS)
                trial, back = copy.deepcopy(model), dataclasses.replace(step)
                for s in others:
                    trial.call(dataclasses.replace(step, stream=s))
                trial.call(back)
                if back.cause == "scratch eviction" or not spec.scratch:
                    break
            pending = [("visit", dataclasses.replace(step, stream=s)) for s in others[1:]] + [("return", home), ("repeat", home)]
            step.stream = others[0]
            step.kind = "churn"
        elif kind == "overflow":  # this call, as many others as there are plans kept, then this one again
            home, others, seen = dataclasses.replace(step), [], {model.key(step)}
            while len(others) < PLAN_CAPACITY:
                other = dataclasses.replace(step, slots={f: r.randrange(SLOTS) for f in spec.fields},
                                            origin={f: r.randrange(2) for f in spec.fields})
                if model.key(other) not in seen and model.key(other) not in model.plans:
                    seen.add(model.key(other))
                    others.append(("visit", other))
            pending = others + [("return", home), ("repeat", home)]
        if kind not in ("refused", "repeat"):
            step.path = r.choice(PATHS)  # (no part of any key)
        if step.mutation:
            model.mutate(*step.mutation)
        model.call(step)
        steps.append(step)
        if not step.same_as:
            history.append(step)
            prev = step
            # a miss is followed by the same call again, most of the time: this is what a cache is for
            room = len(steps) + len(agenda) + 16 * sum(k in long for k in agenda) + 4 < length
            if not step.hit and not pending and (step.cause not in followed or (room and r.random() < 0.3)):
                pending = [("repeat", step)]
                followed.add(step.cause)
            # ... and now and then by the call whose plan the capacity has just pushed out
            elif not pending and room and r.random() < 0.25:
                lost = [k for k, why in model.gone.items() if why == "capacity eviction"]
                for old in reversed(history):
                    if lost and model.key(old) in lost:
                        pending = [("return", old), ("repeat", old)]
                        break
    return steps


def census(spec: Spec, sequences: List[List[Step]]) -> Dict[str, Any]:
    out = {"steps": 0, "hits": 0, "may miss": 0, "kinds": dict.fromkeys(spec.kinds(), 0), "causes": dict.fromkeys(spec.causes(), 0),
           "hit after": dict.fromkeys(spec.causes(), 0), "paths": dict.fromkeys(PATHS, 0), "cold": 0}
    for steps in sequences:
        for n, step in enumerate(steps):
            out["steps"] += 1
            out["hits"] += step.hit
            out["may miss"] += step.may_miss
            out["paths"][step.path] += 1
            if step.kind in out["kinds"]:
                out["kinds"][step.kind] += 1
            if step.cause == "cold" or step.cause == "arrays":
                out["cold"] += 1
            elif step.cause is not None and not step.refused:
                out["causes"][step.cause] += 1
                if n + 1 < len(steps) and steps[n + 1].hit:
                    out["hit after"][step.cause] += 1
    return out
