"""Byte-level DFA constraints on the device (include/glb.h glb_dfa_*).

`ByteDFA` is the automaton a user brings (a compiled regex, a literal set, a schema: a transition table over bytes);
`DeviceConstraint` keeps it on the GPU beside the vocabulary's byte strings and produces what the fused step consumes:
a bank of token bit masks, one row per automaton state that some particle has reached, and every particle's row.  States
advance on the device from the tokens drawn; nothing crosses the host per step.

`ByteWFSA` is the same automaton in the log semiring (arc and final log-weights): a `DeviceConstraint` over one
keeps a bank of float32 rows - the token log-weights from every state reached - that the step adds to the log-probabilities.

`DeviceConstraint(..., on_full="evict")` lets the bank be smaller than the automaton: a cache over the states,
the least recently requested rows recycled and filled again on the device.

`product(llm, a, b, op)` makes the automaton of two automata's conjunction, union or difference on the device,
for `DeviceConstraint(..., minimize=True)` to shrink and serve.

`ByteNFA` is a byte automaton with empty arcs - the union of any number of automata, their concatenation, their closure, a
pattern's Thompson automaton - and `determinize(llm, nfa)` its `ByteDFA`, by the subset construction on the device.

`LazyConstraint` serves a `ByteNFA` as it is: the subset states are made on the device when a particle reaches
them, so a pattern whose deterministic automaton is too large to build still constrains a population that visits little of it.

`BytePDA` is a real-time deterministic pushdown automaton over bytes - nested brackets, `BytePDA.json()` - and `PDAConstraint`
serves one: a state is a configuration, the automaton's state and a bounded stack, numbered on the device when
a particle reaches it.

`ConstraintProduct(llm, parts)` serves the conjunction of 2 to 8 constraints of any of these kinds, products included (DESIGN.md
§26), without building a product automaton: a state is the tuple of the parts' states, numbered on the device when a particle
reaches it, and its row is combined from the parts' rows - the AND of bit rows, the sum of weighted rows with -inf where an
unweighted part forbids the token.  A grammar with a pattern, a length bound and the soft preferences of a `ByteWFSA`.
"""
from .automata import ByteDFA, ByteWFSA  # noqa: F401
from .conj import ConstraintProduct  # noqa: F401
from .device import DeviceConstraint  # noqa: F401
from .lazy import LazyConstraint  # noqa: F401
from .nfa import ByteNFA  # noqa: F401
from .pda import BytePDA, PDAConstraint  # noqa: F401
from .regex import _regex_dfa  # noqa: F401
from .tables import DeviceTables, _kept, determinize, minimize, product  # noqa: F401
