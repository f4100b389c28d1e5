"""What include/sdnq_hip.h declares, read with plain regexes of the tests' own: sdnq_amd/_abi.py is code under test and is not used here."""
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def header_text():
    with open(os.path.join(INCLUDE, "sdnq_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def declared_symbols():
    return sorted(set(re.findall(r"\b(sdnq_hip_[a-z0-9_]+)\s*\(", header_text())))


def declared_arity():  # {entry point: number of parameters} for every prototype
    protos = re.finditer(r"\b(sdnq_hip_[a-z0-9_]+)\s*\(([^;]*)\)\s*;", header_text())
    return {m.group(1): 0 if m.group(2).strip() == "void" else len([a for a in m.group(2).split(",") if a.strip()]) for m in protos}


def struct_field_names(struct):
    hdr = header_text()
    body = hdr[hdr.index("typedef struct %s {" % struct):hdr.index("} %s;" % struct)].split("{", 1)[1]
    return [name.replace("*", " ").split()[-1] for decl in body.split(";") if decl.strip() for name in decl.split(",")]
