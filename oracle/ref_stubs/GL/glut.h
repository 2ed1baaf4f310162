// stand-in for <GL/glut.h> when the reference's front end is compiled against include/ (oracle/Makefile, target ref); prototypes only
#pragma once
#define GLUT_RGB 0
#define GLUT_DOUBLE 2
#define GLUT_LEFT_BUTTON 0
#define GLUT_DOWN 0
#define GL_COLOR_BUFFER_BIT 0x4000
#define GL_DEPTH_BUFFER_BIT 0x100
#define GL_LINES 1
#define GL_POINTS 0
#define GL_POINT_SMOOTH 0xB10
#define GL_DEPTH_TEST 0xB71
#define GL_PROJECTION 0x1701
#define GL_MODELVIEW 0x1700
extern "C" {
void glutInit(int *, char **); void glutInitDisplayMode(unsigned); void glutInitWindowSize(int, int);
int glutCreateWindow(const char *); void glutDisplayFunc(void (*)()); void glutMouseFunc(void (*)(int, int, int, int));
void glutMainLoop(); void glutSwapBuffers(); void glutPostRedisplay();
void glClear(unsigned); void glLoadIdentity(); void glColor3f(float, float, float); void glBegin(unsigned); void glEnd();
void glVertex3fv(const float *); void glVertex3f(float, float, float); void glClearColor(float, float, float, float);
void glEnable(unsigned); void glPointSize(float); void glMatrixMode(unsigned);
void glFrustum(double, double, double, double, double, double); void glTranslatef(float, float, float);
}
