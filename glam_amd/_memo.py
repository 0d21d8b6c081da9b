"""The weak per-tensor side table of the host path: data derived from a tensor, remembered until the tensor dies or is written in place."""
import weakref


class TensorMemo:
    """``key="id"``: one entry per tensor object; ``key="ptr"``: one per ``data_ptr()``, so another tensor object over the same memory
    finds it too.  An entry is ``(weakref, the tensor's _version at registration, value)``.  What else a hit depends on (a shape, a width,
    a dropout rate) the caller checks on the value it gets back."""

    def __init__(self, key):
        self._key = {"id": id, "ptr": lambda t: t.data_ptr()}[key]
        self._d = {}

    def put(self, t, value):
        key = self._key(t)

        def gone(ref, k=key, d=self._d):
            hit = d.get(k)
            # ids and addresses come back: a newer tensor under this key keeps its entry.  (A replaced entry takes its weakref along, and
            # a dead weakref calls nothing, so this holds as long as the entry is the weakref's only owner; the check does not rely on it.)
            if hit is not None and hit[0] is ref:
                del d[k]
        try:
            self._d[key] = (weakref.ref(t, gone), t._version, value)
        except TypeError:                              # no weak references to this object: not remembered
            pass

    def get(self, t, same_object=True):
        """The value registered for ``t`` — with ``same_object=False`` for any live tensor under ``t``'s key — unwritten since, else None."""
        hit = self._d.get(self._key(t))
        if hit is None or hit[1] != t._version:
            return None
        live = hit[0]()
        if live is None or (same_object and live is not t):
            return None
        return hit[2]

    def take(self, t, same_object=True):
        """``get``; a hit leaves the table."""
        value = self.get(t, same_object)
        if value is not None:
            del self._d[self._key(t)]
        return value

    def referent(self, t):
        """The live, unwritten tensor registered under ``t``'s key, or None."""
        hit = self._d.get(self._key(t))
        live = hit[0]() if hit is not None else None
        return live if live is not None and live._version == hit[1] else None

    def __len__(self):
        return len(self._d)

    def clear(self):
        self._d.clear()
