"""The one mechanism behind every module's ``install`` / ``uninstall``: set attributes on one of the reference's classes or modules
and put back exactly what was there."""
from __future__ import annotations

from typing import Callable, Dict, Mapping, Optional

MISSING = object()      # the target's own __dict__ did not hold the name


class Seam:
    """One per module, so ``uninstall()`` without arguments undoes that module's patches only.  Everything is read from and recorded
    for ``target.__dict__``, never through inheritance: a subclass does not see its base class's patch as its own."""

    def __init__(self):
        self._former: Dict[object, Dict[str, object]] = {}      # target -> {name: what its __dict__ held before the first install}

    def install(self, target, functions: Mapping[str, Callable], reference: Optional[str] = None) -> None:
        """Sets ``target.<name>`` for every entry of ``functions``.  ``reference``: an attribute that receives, in ``target``'s own
        ``__dict__``, what ``target.<name>`` resolved to before the first install -- its own or an inherited one."""
        former = self._former.setdefault(target, {})
        for name, fn in functions.items():
            if name not in former:
                former[name] = target.__dict__.get(name, MISSING)
                if reference is not None:               # (recorded and put back like any other attribute)
                    former.setdefault(reference, target.__dict__.get(reference, MISSING))
                    setattr(target, reference, getattr(target, name, None))
            setattr(target, name, fn)

    def former(self, target, name: str):
        """What ``target.__dict__`` held under ``name`` before the first install (``MISSING``: nothing)."""
        return self._former[target][name]

    def uninstall(self, *targets) -> None:
        """Puts back what ``install`` replaced (no target given: on every one of this seam's); a target never installed is left alone."""
        for target in (targets or tuple(self._former)):
            for name, old in self._former.pop(target, {}).items():
                if old is not MISSING:
                    setattr(target, name, old)
                elif name in target.__dict__:
                    delattr(target, name)
