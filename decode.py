#!/usr/bin/env python3
"""Drop-in for the reference's decode.py (same flags): see scp_amd/cli.py decode_octattn_main."""
from scp_amd.cli import decode_octattn_main

if __name__ == "__main__":
    decode_octattn_main()
