"""The switch table of the bundle-adjustment unit (mvus_amd/csrc/ba_switches.h), on the host build of tests/hostcheck: every field's
documented default, what each MVUS_* variable does to its field, and that the table is complete -- no other file of the unit reads
the environment."""
import glob
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mvus_amd', 'csrc')

# variable: (default, value to set, field with that value).  bools read as 0 / 1
TABLE = {
    'MVUS_LM_NO_CARRY': (0, '1', 1), 'MVUS_FETCH_EVENT': (0, '1', 1), 'MVUS_NO_SPEC_SHARDS': (0, '1', 1), 'MVUS_SQ_DEVICE_SUM': (0, '1', 1),
    'MVUS_LSMR_HOST': (0, '1', 1), 'MVUS_LSMR_BOUNDED_HOST': (0, '1', 1), 'MVUS_LSMR_ONE_PASS': (0, '1', 1), 'MVUS_LSMR_TRACE': (0, '1', 1),
    'MVUS_GEMM_SLABS': (0, '3', 3), 'MVUS_RCS': (0, 'gj', 1), 'MVUS_RCS_TRSM': (0, 'launch', 1),
    'MVUS_RCS_SPIN_LIMIT': (-1, '0', 0),              # zero is a value (the first poll gives up), not "unset"
    'MVUS_BCR_FUSED': (1, '0', 0), 'MVUS_PART_LEN': (0, '16', 16), 'MVUS_PART_BACK': (0, '1', 1), 'MVUS_DIRECT_RHS': (1, '0', 0),
    'MVUS_SEP_SEQUENTIAL': (0, '1', 1), 'MVUS_SEP_TWO_LEVEL': (1, '0', 0), 'MVUS_ASM_ATOMIC': (0, '1', 1), 'MVUS_WIN': (0, '9', 9),
    'MVUS_WIN_GROUPS': (0, '2', 2), 'MVUS_NO_SPEC': (0, '1', 1), 'MVUS_LM_MATERIALIZE_J': (0, '1', 1), 'MVUS_NE_FROM_J': (0, '1', 1),
    'MVUS_NO_OVERLAP': (0, '1', 1), 'MVUS_DEBUG': (0, '1', 1),
}
# read outside the table, by design: the roctx ranges of api_common.h and the spline unit's own switches (MVUS_DEBUG there is the table's name)
OUTSIDE = {'MVUS_ROCTX', 'MVUS_BAND_PARTS_SCALE', 'MVUS_FIT_SLICES_MAX', 'MVUS_BAND_PARTS_MIN', 'MVUS_FIT_TIMING', 'MVUS_DEBUG'}
BA_FILES = ('ba_api.hip', 'ba_backend.hip.h', 'ba_schur_host.hip.h', 'ba_schur.h', 'ba_solver.h')


@pytest.fixture
def switch(monkeypatch):
    import hostcheck_util
    lib = hostcheck_util.load()
    for name in TABLE:
        monkeypatch.delenv(name, raising=False)
    return lambda name: lib.hostcheck_switch(name.encode())


def test_defaults_with_nothing_set(switch):
    for name, (default, _, _) in TABLE.items():
        assert switch(name) == default, name
    assert switch('MVUS_NO_SUCH_SWITCH') == -2


@pytest.mark.parametrize('name', sorted(TABLE))
def test_each_variable_moves_its_field_and_no_other(name, switch, monkeypatch):
    default, text, value = TABLE[name]
    monkeypatch.setenv(name, text)
    assert value != default and switch(name) == value
    for other, (d, _, _) in TABLE.items():
        if other != name:
            assert switch(other) == d, (name, other)
    monkeypatch.delenv(name)
    assert switch(name) == default


@pytest.mark.parametrize('name,text,value', [
    ('MVUS_WIN', '0', 0), ('MVUS_WIN', '-3', 0), ('MVUS_WIN_GROUPS', '0', 0), ('MVUS_GEMM_SLABS', '0', 0),       # not positive: reads as unset
    ('MVUS_RCS', 'ldlt', 0), ('MVUS_RCS_TRSM', '1', 0),                                                          # only the one word counts
    ('MVUS_BCR_FUSED', '1', 1), ('MVUS_SEP_TWO_LEVEL', '1', 1), ('MVUS_DIRECT_RHS', '1', 1),                       # switched on by number
    ('MVUS_RCS_SPIN_LIMIT', '100', 100), ('MVUS_PART_BACK', '0', 1), ('MVUS_ASM_ATOMIC', '', 1),                   # flags count when set, whatever the text
    ('MVUS_PART_LEN', '0', 1),                                                                                    # set: the shortest interior, not the default
])
def test_parsing_at_the_edges(name, text, value, switch, monkeypatch):
    monkeypatch.setenv(name, text)
    assert switch(name) == value


def _getenv_names(path):
    with open(path) as f:
        return set(re.findall(r'getenv\(\s*"(MVUS_[A-Z0-9_]+)"', f.read()))


def test_the_table_is_complete():
    """Every MVUS_* variable the library reads is a row of the table or one of the reads left outside it on purpose; the four
    files of the BA unit do not touch the environment at all."""
    with open(os.path.join(CSRC, 'ba_switches.h')) as f:
        header = f.read()
    in_header = set(re.findall(r'"(MVUS_[A-Z0-9_]+)"', header))
    assert in_header == set(TABLE)
    for name in TABLE:                                  # documented: every variable is named in a member's comment as well
        assert re.search(r'//\s*%s\b' % name, header), name
    sources = [p for p in glob.glob(os.path.join(CSRC, '*')) if p.endswith(('.h', '.hip', '.cpp'))]
    assert len(sources) > 10
    elsewhere = set()
    for p in sources:
        if os.path.basename(p) == 'ba_switches.h':
            continue
        with open(p) as f:
            text = f.read()
        if os.path.basename(p) in BA_FILES:
            assert 'getenv' not in text, os.path.basename(p)
        # every read names its variable in place: nothing reaches getenv through a variable
        assert len(re.findall(r'\bgetenv\s*\(', text)) == len(re.findall(r'\bgetenv\(\s*"MVUS_[A-Z0-9_]+"', text)), os.path.basename(p)
        elsewhere |= _getenv_names(p)
    assert elsewhere == OUTSIDE
