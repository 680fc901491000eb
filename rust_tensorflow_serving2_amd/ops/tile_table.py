"""Reader of ``kernels/tile_configs.h``, the one place the tile configs are
written down: the ``X(...)`` rows of each ``#define TFSK_<FAMILY>_CONFIGS(X)``
list, as tuples of ints in file order."""
import os
import re
from typing import Dict, List, Tuple

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kernels", "tile_configs.h")
# columns per row of each list (see the header)
FAMILIES = {"IGEMM": 7, "CGEMM": 6, "CGEMM_PF": 7, "CGEMM32": 6, "BGEMM": 3, "HALO": 8, "HALO_PERSIST": 4}


def read_rows(path: str = HEADER) -> Dict[str, List[Tuple[int, ...]]]:
    """{family: [row, ...]}; ImportError when the header is missing or is not
    the lists ``FAMILIES`` names (there is no second copy to fall back to)."""
    try:
        with open(path) as f:
            text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
        out = {}
        for name, body in re.findall(r"^#define TFSK_(\w+)_CONFIGS\(X\)((?:.*\\\n)*.*)", text, flags=re.M):
            calls = re.findall(r"X\(([^()]*)\)", body)
            if not calls or re.sub(r"X\([^()]*\)|\\", "", body).strip():
                raise ValueError(f"TFSK_{name}_CONFIGS is not a list of X(...) rows")
            out[name] = [tuple(int(v) for v in c.split(",")) for c in calls]
        if {k: {len(r) for r in v} for k, v in out.items()} != {k: {n} for k, n in FAMILIES.items()}:
            raise ValueError("the lists or their columns are not " + repr(FAMILIES))
    except (OSError, ValueError) as e:
        raise ImportError(f"cannot read the tile configs from {path}: {e!r}") from e
    return out
