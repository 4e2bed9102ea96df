"""The mesh file writers (infinitam_amd/csrc/mesh_files.h: write_ply / write_obj / write_stl on a host-side view of a mesh) without a GPU.

A stand-alone program that includes mesh_files.h and nothing else of the library is compiled with the address and undefined-behaviour
sanitizers and writes every format for the soup and the indexed form of two triangles that share an edge, with and without attributes,
and for empty meshes.  The expected bytes are built here from the formats' definitions -- literal header text, struct.pack, '%f' -- and
whole files are compared for equality; the program must end with status 0 and nothing on stderr.  A path in a directory that does not
exist must give "cannot create <path>" and leave nothing behind."""
import os
import struct
import subprocess

import numpy as np
import pytest

import itm_testlib as T

F = np.float32
HEADER = os.path.join(T.ROOT, "infinitam_amd", "csrc", "mesh_files.h")

# four vertices, two triangles over the edge (1, 2); a negative coordinate, values with more than six decimals, one that rounds up in '%f'
VERTICES = np.array([[0.0, 0.0, 0.0], [1.25, 0.0, -0.5], [0.1234567, 1.0, 0.33333334], [1.0, 1.0000005, -2.7500007]], F)
FACES = np.array([[0, 1, 2], [2, 1, 3]], np.uint32)
NORMALS = np.array([[0.0, 0.0, 1.0], [-0.6, 0.8, 0.0], [0.57735026, -0.57735026, 0.57735026], [0.0, 0.0, 0.0]], F)
COLOURS = np.array([[255, 0, 17, 201], [1, 2, 3, 202], [128, 127, 126, 203], [9, 250, 77, 204]], np.uint8)    # the fourth byte is not written
SOUP = FACES.reshape(-1)                                   # the soup's vertex j is vertex SOUP[j] of the four
EMPTY3 = np.zeros((0, 3), F)


def case(name, positions, faces, normals=None, colours=None):
    return {"name": name, "positions": positions, "faces": faces, "normals": normals, "colours": colours}


CASES = [
    case("empty_soup", EMPTY3, None),
    case("empty_indexed", EMPTY3, np.zeros((0, 3), np.uint32), EMPTY3, np.zeros((0, 4), np.uint8)),
    case("soup_nc", VERTICES[SOUP], None, NORMALS[SOUP], COLOURS[SOUP]),
    case("soup", VERTICES[SOUP], None),
    case("indexed", VERTICES, FACES),
    case("indexed_n", VERTICES, FACES, NORMALS, None),
    case("indexed_c", VERTICES, FACES, None, COLOURS),
    case("indexed_nc", VERTICES, FACES, NORMALS, COLOURS),
]


# ---- the formats, from their definitions -------------------------------------------------------------------------------------------

def faces_of(c):
    """the soup's face i is (3i, 3i + 1, 3i + 2)"""
    return c["faces"] if c["faces"] is not None else np.arange(len(c["positions"]), dtype=np.uint32).reshape(-1, 3)


def expected_ply(c):
    pos, faces = c["positions"], faces_of(c)
    head = "ply\nformat binary_little_endian 1.0\ncomment itm-hip mesh\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(pos)
    if c["normals"] is not None:
        head += "property float nx\nproperty float ny\nproperty float nz\n"
    if c["colours"] is not None:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(faces)
    out = head.encode("ascii")
    for v in range(len(pos)):
        out += struct.pack("<3f", *pos[v])
        if c["normals"] is not None:
            out += struct.pack("<3f", *c["normals"][v])
        if c["colours"] is not None:
            out += struct.pack("<3B", *c["colours"][v][:3])
    for f in faces:
        out += struct.pack("<B3i", 3, int(f[2]), int(f[1]), int(f[0]))          # the winding reversed
    return out


def expected_obj(c):
    lines = ["v %f %f %f\n" % tuple(float(x) for x in p) for p in c["positions"]]
    lines += ["f %d %d %d\n" % (int(f[2]) + 1, int(f[1]) + 1, int(f[0]) + 1) for f in faces_of(c)]    # 1-based, the winding reversed
    return "".join(lines).encode("ascii")


def expected_stl(c):
    pos, faces = c["positions"], faces_of(c)
    out = b" " * 80 + struct.pack("<I", len(faces))
    for f in faces:
        out += struct.pack("<3f", 0.0, 0.0, 0.0)
        for k in (2, 1, 0):
            out += struct.pack("<3f", *pos[int(f[k])])
        out += struct.pack("<H", 0)
    return out


EXPECTED = {"ply": expected_ply, "obj": expected_obj, "stl": expected_stl}


# ---- the program -------------------------------------------------------------------------------------------------------------------

def c_array(ctype, name, values, literal):
    body = ", ".join(literal(v) for v in values) if len(values) else literal(0)     # (an empty case still names an array: no zero-length array)
    return "static const %s %s[] = {%s};\n" % (ctype, name, body)


def program_source():
    src = '#include "mesh_files.h"\n\n#include <cstdio>\n#include <string>\n\n'
    calls = ""
    for c in CASES:
        n = c["name"]
        src += c_array("float", n + "_positions", c["positions"].reshape(-1), lambda v: float(v).hex() + "f")
        if c["faces"] is not None:
            src += c_array("uint32_t", n + "_faces", c["faces"].reshape(-1), lambda v: "%du" % int(v))
        if c["normals"] is not None:
            src += c_array("float", n + "_normals", c["normals"].reshape(-1), lambda v: float(v).hex() + "f")
        if c["colours"] is not None:
            src += c_array("uint8_t", n + "_colours", c["colours"].reshape(-1), lambda v: "%d" % int(v))
        calls += "  {\n    itm::HostMesh m;\n    m.positions = %s_positions; m.noVertices = %d; m.noTriangles = %d;\n" % (n, len(c["positions"]), len(faces_of(c)))
        if c["faces"] is not None:
            calls += "    m.faces = %s_faces;\n" % n
        if c["normals"] is not None:
            calls += "    m.withNormals = true; m.normals = %s_normals;\n" % n
        if c["colours"] is not None:
            calls += "    m.withColours = true; m.colours = %s_colours;\n" % n
        calls += '    failures += all_formats(m, dir + "/%s");\n  }\n' % n
    src += """
static int report(const std::string& error, const std::string& path) {
  if (!error.empty()) printf("%s: %s\\n", path.c_str(), error.c_str());
  return error.empty() ? 0 : 1;
}

static int all_formats(const itm::HostMesh& m, const std::string& stem) {
  return report(itm::write_ply(m, (stem + ".ply").c_str()), stem + ".ply") + report(itm::write_obj(m, (stem + ".obj").c_str()), stem + ".obj") +
         report(itm::write_stl(m, (stem + ".stl").c_str()), stem + ".stl");
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = argv[1];
  int failures = 0;
""" + calls + """  {  // the last case again, into a directory that does not exist: every writer must say so
    itm::HostMesh m;
    m.positions = indexed_nc_positions; m.noVertices = 4; m.noTriangles = 2; m.faces = indexed_nc_faces;
    const std::string missing = dir + "/no_such_directory/mesh";
    for (const std::string& error : {itm::write_ply(m, (missing + ".ply").c_str()), itm::write_obj(m, (missing + ".obj").c_str()),
                                     itm::write_stl(m, (missing + ".stl").c_str())})
      printf("missing: %s\\n", error.c_str());
  }
  return failures ? 1 : 0;
}
"""
    return src


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """the directory the sanitized program wrote into, and its standard output"""
    work = tmp_path_factory.mktemp("mesh_files")
    src, exe, out = work / "mesh_files_main.cpp", work / "mesh_files_main", work / "out"
    out.mkdir()
    src.write_text(program_source())
    # (the sanitizers' runtimes linked into the program itself: it stands alone)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                    "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True, capture_output=True)
    res = subprocess.run([str(exe), str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stderr == "", res.stderr                    # nothing from either sanitizer
    return out, res.stdout


def test_header_is_plain_cpp():
    text = open(HEADER).read()
    assert "hip" not in text.replace("itm-hip mesh", "").lower()
    assert [line for line in text.splitlines() if line.startswith("#include")] == [
        "#include <cstdint>", "#include <cstdio>", "#include <cstring>", "#include <string>", "#include <vector>"]


@pytest.mark.parametrize("fmt", ["ply", "obj", "stl"])
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_file_is_the_format_byte_for_byte(written, c, fmt):
    out, _ = written
    got = (out / (c["name"] + "." + fmt)).read_bytes()
    want = EXPECTED[fmt](c)
    assert got == want, f"{c['name']}.{fmt}: {len(got)} bytes written, {len(want)} expected"


def test_formatting_is_exercised():
    """what the cases are there for: a sign, digits beyond the sixth decimal (one of them rounding up), a dropped fourth colour byte"""
    text = expected_obj(CASES[4]).decode()
    assert "v 1.250000 0.000000 -0.500000\n" in text and "v 0.123457 1.000000 0.333333\n" in text and "v 1.000000 1.000000 -2.750001\n" in text
    assert text.endswith("f 3 2 1\nf 4 2 3\n")
    assert expected_obj(CASES[3]).decode().endswith("f 3 2 1\nf 6 5 4\n")
    assert len(expected_ply(CASES[7])) - len(expected_ply(CASES[5])) == 4 * 3 + len("property uchar red\nproperty uchar green\nproperty uchar blue\n")


def test_missing_directory_is_reported_and_leaves_nothing(written):
    out, stdout = written
    missing = str(out / "no_such_directory" / "mesh")
    assert stdout.splitlines() == ["missing: cannot create " + missing + e for e in (".ply", ".obj", ".stl")]
    assert not os.path.exists(os.path.dirname(missing))
    assert sorted(os.listdir(out)) == sorted(c["name"] + "." + e for c in CASES for e in EXPECTED)
