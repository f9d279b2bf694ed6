"""Start a ThreadSanitizer build with address-space randomisation off for that process.

TSan's runtime places its shadow at fixed addresses and ends the program at start-up ("FATAL: ThreadSanitizer:
unexpected memory mapping") when the kernel has put the executable or a library where the shadow layout does not expect
one, which happens on hosts that randomise mappings with more bits than the runtime was built for (vm.mmap_rnd_bits =
32).  `preexec_fn=noaslr.no_aslr` sets ADDR_NO_RANDOMIZE in the child's personality before it executes the program, as
`setarch -R` does; the flag belongs to that process alone.
"""
import ctypes

ADDR_NO_RANDOMIZE = 0x0040000
_libc = ctypes.CDLL(None, use_errno=True)


def no_aslr():
    persona = _libc.personality(0xFFFFFFFF)  # query
    if persona != -1:
        _libc.personality(persona | ADDR_NO_RANDOMIZE)
