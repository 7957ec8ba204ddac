// db_tab.h -- written by tools/gen_db_term_table.py 6 5; do not edit.  The constants of db_term_fast (db_spec.h).
#pragma once
#define HPFW_DB_CELL_BITS 6
#define HPFW_DB_DEGREE 5
// 10 log10(2)
#define HPFW_DB_LOG2 0x1.8151824c7587fp+1
// (-1)^(k+1) (10 / ln 10) / k, k = 1 .. degree: 10 log10(1 + r) = sum of these times r^k
#define HPFW_DB_POLY { 0x1.15f2ced384f29p+2, -0x1.15f2ced384f29p+1, 0x1.729913c4b1436p+0, -0x1.15f2ced384f29p+0, 0x1.bcb7b1526e50ep-1 }
// cell i: { 1 / c_i, 10 log10(c_i) }, c_i = 1 + (i + 1/2) / 64
#define HPFW_DB_TABLE { \
    { 0x1.fc07f01fc07f0p-1, 0x1.14de4c7553438p-5 }, \
    { 0x1.f44659e4a4271p-1, 0x1.9c1ca65954425p-4 }, \
    { 0x1.ecc07b301ecc0p-1, 0x1.54d2492558796p-3 }, \
    { 0x1.e573ac901e574p-1, 0x1.d9934d709e7f6p-3 }, \
    { 0x1.de5d6e3f8868ap-1, 0x1.2e3042bf62379p-2 }, \
    { 0x1.d77b654b82c34p-1, 0x1.6ea43713b3d9ep-2 }, \
    { 0x1.d0cb58f6ec074p-1, 0x1.ae2c72a6028d1p-2 }, \
    { 0x1.ca4b3055ee191p-1, 0x1.eccf9966659f0p-2 }, \
    { 0x1.c3f8f01c3f8f0p-1, 0x1.154a04378be73p-1 }, \
    { 0x1.bdd2b899406f7p-1, 0x1.33bfecf317505p-1 }, \
    { 0x1.b7d6c3dda338bp-1, 0x1.51cc744e15bf6p-1 }, \
    { 0x1.b2036406c80d9p-1, 0x1.6f7269b662f9cp-1 }, \
    { 0x1.ac5701ac5701bp-1, 0x1.8cb4803367dd7p-1 }, \
    { 0x1.a6d01a6d01a6dp-1, 0x1.a9954fdfd0e26p-1 }, \
    { 0x1.a16d3f97a4b02p-1, 0x1.c617574b0db7cp-1 }, \
    { 0x1.9c2d14ee4a102p-1, 0x1.e23cfcc470d5cp-1 }, \
    { 0x1.970e4f80cb872p-1, 0x1.fe088f919ca8cp-1 }, \
    { 0x1.920fb49d0e229p-1, 0x1.0cbe2488e36c4p+0 }, \
    { 0x1.8d3018d3018d3p-1, 0x1.1a4d26e79c55fp+0 }, \
    { 0x1.886e5f0abb04ap-1, 0x1.27b257402aa01p+0 }, \
    { 0x1.83c977ab2beddp-1, 0x1.34eeb47ca9743p+0 }, \
    { 0x1.7f405fd017f40p-1, 0x1.42033487de1a8p+0 }, \
    { 0x1.7ad2208e0ecc3p-1, 0x1.4ef0c4b85b523p+0 }, \
    { 0x1.767dce434a9b1p-1, 0x1.5bb84a357c453p+0 }, \
    { 0x1.724287f46debcp-1, 0x1.685aa256a2955p+0 }, \
    { 0x1.6e1f76b4337c7p-1, 0x1.74d8a2fd1a8b4p+0 }, \
    { 0x1.6a13cd1537290p-1, 0x1.81331ae900bc9p+0 }, \
    { 0x1.661ec6a5122f9p-1, 0x1.8d6ad2097d766p+0 }, \
    { 0x1.623fa77016240p-1, 0x1.998089c8a3d16p+0 }, \
    { 0x1.5e75bb8d015e7p-1, 0x1.a574fd533c74cp+0 }, \
    { 0x1.5ac056b015ac0p-1, 0x1.b148e1dcbeb38p+0 }, \
    { 0x1.571ed3c506b3ap-1, 0x1.bcfce6dfb5c29p+0 }, \
    { 0x1.5390948f40febp-1, 0x1.c891b65acb485p+0 }, \
    { 0x1.5015015015015p-1, 0x1.d407f50aac626p+0 }, \
    { 0x1.4cab88725af6ep-1, 0x1.df6042a0fa747p+0 }, \
    { 0x1.49539e3b2d067p-1, 0x1.ea9b39f87595fp+0 }, \
    { 0x1.460cbc7f5cf9ap-1, 0x1.f5b971468b3d6p+0 }, \
    { 0x1.42d6625d51f87p-1, 0x1.005dbd25386b9p+1 }, \
    { 0x1.3fb013fb013fbp-1, 0x1.05d0f13cf79c3p+1 }, \
    { 0x1.3c995a47babe7p-1, 0x1.0b36999600afep+1 }, \
    { 0x1.3991c2c187f63p-1, 0x1.108ef8e0b3504p+1 }, \
    { 0x1.3698df3de0748p-1, 0x1.15da4fe5a31a8p+1 }, \
    { 0x1.33ae45b57bcb2p-1, 0x1.1b18dd98001a5p+1 }, \
    { 0x1.30d190130d190p-1, 0x1.204adf27230d6p+1 }, \
    { 0x1.2e025c04b8097p-1, 0x1.2570900f49aa6p+1 }, \
    { 0x1.2b404ad012b40p-1, 0x1.2a8a2a298e5fap+1 }, \
    { 0x1.288b01288b013p-1, 0x1.2f97e5bb26409p+1 }, \
    { 0x1.25e22708092f1p-1, 0x1.3499f983ef2edp+1 }, \
    { 0x1.23456789abcdfp-1, 0x1.39909acc57a84p+1 }, \
    { 0x1.20b470c67c0d9p-1, 0x1.3e7bfd72a9106p+1 }, \
    { 0x1.1e2ef3b3fb874p-1, 0x1.435c53f7bcbedp+1 }, \
    { 0x1.1bb4a4046ed29p-1, 0x1.4831cf8b239ccp+1 }, \
    { 0x1.19453808ca29cp-1, 0x1.4cfca016c7a1fp+1 }, \
    { 0x1.16e0689427379p-1, 0x1.51bcf44a0e11fp+1 }, \
    { 0x1.1485f0e0acd3bp-1, 0x1.5672f9a480f2dp+1 }, \
    { 0x1.12358e75d3033p-1, 0x1.5b1edc8005d37p+1 }, \
    { 0x1.0fef010fef011p-1, 0x1.5fc0c81aa79e6p+1 }, \
    { 0x1.0db20a88f4696p-1, 0x1.6458e69ff8df7p+1 }, \
    { 0x1.0b7e6ec259dc8p-1, 0x1.68e7613213946p+1 }, \
    { 0x1.0953f39010954p-1, 0x1.6d6c5ff23b568p+1 }, \
    { 0x1.073260a47f7c6p-1, 0x1.71e80a0926641p+1 }, \
    { 0x1.05197f7d73404p-1, 0x1.765a85aef1d2bp+1 }, \
    { 0x1.03091b51f5e1ap-1, 0x1.7ac3f832c4f2ep+1 }, \
    { 0x1.0101010101010p-1, 0x1.7f24860227b7bp+1 }, \
}
