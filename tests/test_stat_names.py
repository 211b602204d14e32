"""CPU checks of the counter-slot table (fi_types.h FI_STAT_SLOTS) through
fi_debug_stat_name, which needs no device: the names shrewd_amd.STAT is made
of, and the slot numbers that bench.py, the histogram kernel and the dumps
under profiles/ read by number."""
import ctypes


def stat_names():
    from shrewd_amd import build_library
    lib = ctypes.CDLL(build_library())
    lib.fi_debug_stat_name.restype = ctypes.c_char_p
    lib.fi_debug_stat_name.argtypes = [ctypes.c_uint32]
    return lib, {i: lib.fi_debug_stat_name(i).decode() for i in range(64) if lib.fi_debug_stat_name(i)}


def test_stat_names_unique_and_cover_the_written_slots():
    _, names = stat_names()
    assert len(set(names.values())) == len(names)
    used = set(range(0, 28)) | {30} | set(range(32, 63))
    assert set(names) == used


def test_stat_slots_read_by_number_keep_their_numbers():
    _, names = stat_names()
    assert (names[0], names[1], names[2], names[23]) == ("FETCH_BYTES", "DATA_BYTES", "PAGES", "DEVICE_INSTS")
    kernels = ("K64", "SOLO", "SOLO_ODD")   # 0 the 64-lane kernel, 1 solo, 2 solo-odd
    fields = ("FETCH_BYTES", "DATA_BYTES", "PAGES", "DEVICE_INSTS")
    for k, kn in enumerate(kernels):
        for off, fn in enumerate(fields):
            assert names[40 + 4 * k + off] == f"{kn}_{fn}"
    assert [names[32 + k] for k in range(8)] == [f"PROF_PHASE{k}" for k in range(8)]


def test_stat_name_null_for_unnamed_slots():
    lib, _ = stat_names()
    for slot in (28, 29, 31, 63, 64, 65, 1 << 16, (1 << 32) - 1):
        assert lib.fi_debug_stat_name(slot) is None, slot


def test_python_enum_is_the_library_table():
    import shrewd_amd
    _, names = stat_names()
    assert {int(s): s.name for s in shrewd_amd.STAT} == names
    assert shrewd_amd.STAT.TX_INSTS == 16 and shrewd_amd.fi.STAT is shrewd_amd.STAT
