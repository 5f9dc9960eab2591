"""The stage table of the Python closed loop (_lib.STAGES) without a GPU and without the library: it agrees with the ladder of
mpcx_closed_loop_run* prototypes in include/mpcx.h, its dependents close to the sets written out here, and an unknown stage keyword is
refused before anything is called.  The device side is tests/test_gpu_stage_switches.py."""
import os
import re

import pytest

from mpc_for_av_at_intersection_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('log', 'opts', 'retire', 'scene', 'admit', 'respawn', 'routes', 'precedence', 'signals', 'actuation', 'advice', 'intent', 'reservation')
# stage -> what goes with it when it is switched off; (stage, True): right of way is on by order of entry
CLOSURE = {
    'retire': {'scene', 'admit', 'respawn', 'routes', 'precedence'},
    'scene': {'admit', 'respawn', 'routes', 'precedence'},
    ('admit', True): {'respawn', 'routes', 'precedence'},
    'admit': {'respawn', 'routes'},
    'respawn': {'routes'},
    'signals': {'actuation', 'reservation', 'advice'},
}


def _ladder():
    """entry point -> the struct names of its `const mpcx_* *` parameters behind the descriptor, as include/mpcx.h declares them"""
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mpcx.h')).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r'\bint32_t\s+(mpcx_closed_loop_run\w*)\s*\(([^)]*)\)\s*;', hdr):
        structs = re.findall(r'const\s+(mpcx_\w+)\s*\*', params)
        assert structs[:2] == ['mpcx_interaction_params', 'mpcx_closed_loop'], name
        out[name] = structs[2:]
    return out


def test_table_is_the_headers_ladder():
    """every mpcx_closed_loop_run* prototype takes, behind the descriptor, the first k structs of the table in the table's order, for
    k = 0 .. 13 once each, and the table's derived entry points are exactly the fourteen declared -- rung k under the name derived for it"""
    assert tuple(st.key for st in _lib.STAGES) == _lib.STAGE_KEYS == KEYS
    c_names = [st.c_name for st in _lib.STAGES]
    ladder = _ladder()
    assert len(ladder) == 14 and sorted(ladder) == sorted(_lib.LOOP_ENTRY_POINTS) and len(set(_lib.LOOP_ENTRY_POINTS)) == 14
    for k, name in enumerate(_lib.LOOP_ENTRY_POINTS):
        assert ladder[name] == c_names[:k], name
    assert all(name in _lib.EXPORTS for name in ladder) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    for st in _lib.STAGES:      # the struct of a row is the mirror of the row's C struct, and every row has its paragraph
        assert ('mirror of %s ' % st.c_name) in st.struct.__doc__ and st.doc.startswith('a _lib.%s -- ' % st.struct.__name__), st.key


@pytest.mark.parametrize('entry', (False, True))
def test_dependents_close_to_the_sets_written_out(entry):
    for key in KEYS:
        want = CLOSURE.get((key, entry), CLOSURE.get(key, set()))
        assert _lib.stage_dependents(key, entry_order=entry) == want, (key, entry)


def test_unknown_stage_keyword_is_a_type_error():
    """the check Context.closed_loop_run makes on its keywords before it touches the library: every stage is a keyword, what is not given
    is None, in the table's order, and anything else is a TypeError that names the stages"""
    given = {'reservation': 3, 'log': 1}
    assert _lib.stage_structs(given) == [1] + [None] * 11 + [3] and _lib.stage_structs({}) == [None] * 13
    with pytest.raises(TypeError, match=r"unexpected keyword argument 'reserve'.*" + ', '.join(KEYS)):
        _lib.stage_structs({'signals': 1, 'reserve': 2})
